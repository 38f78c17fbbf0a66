"""The optimizer step of the training loop (train.py:237,653: Adam(amsgrad=True, weight_decay=1e-5)) in ONE HIP launch for all
parameters of a group: csrc/optim.hip, bmc_adam_step; include/bmc_hip.h "optimizer step" states the arithmetic, rounding by rounding.

`Adam` is a drop-in for the constructor calls this repository and the reference make.  It IS a torch.optim.Optimizer: the global
pre-step hook of bmc_hip.ops (weight gradients on the side stream), GradAllReducer's pre-step hook and LR schedulers work on
it as on torch's, and its state has torch's keys, dtypes and devices -- state_dict() of either optimizer loads into the other.
The class keeps the name `Adam`: checkpoint.resume matches optimizers by type(optimizer).__name__.

What happens per step and group: the parameters that have a gradient and share a step count are cut into chunks of at most 4096
elements of one tensor (chunk_table); the table is built in a pinned buffer, copied to the device once and memoised by the tuple
of all data pointers (the caching allocator repeats addresses: from the second step on usually nothing is copied); one launch
updates p, exp_avg, exp_avg_sq and max_exp_avg_sq in place, 36 bytes per element; the parameters' version counters advance, so
that every cache keyed on them (weight packs, chains, inference graphs) sees the new values.  There is no fallback: what the
kernel does not do (CPU, non-fp32 or non-contiguous parameters, sparse gradients, maximize, ...) raises ValueError.

Clipping (csrc/optim.hip as well; include/bmc_hip.h "optimizer step: clipping").  Adam(..., max_grad_norm=X) clips by the global L2
norm of ALL gradients of the step, as torch.nn.utils.clip_grad_norm_(model.parameters(), X) before step() does, and
nonfinite="skip" leaves parameters and state untouched when any gradient element is Inf or NaN -- both without a host round
trip: one norm launch per step launch writes float64 partials, and every workgroup of the step launches adds them up in one
fixed order to the same coefficient c = min(1, X / (norm + 1e-6)).  Different from torch: `.grad` is NEVER written (the kernel
multiplies while it reads), so gradients that are views of GradAllReducer's flat buckets stay as reduced; the pre-step hooks
(the side-stream join of bmc_hip.ops, the reducer's all-reduce) run before the norm launch, so the norm is that of the
reduced gradients.  A skipped step still counts as a step: `step` advances on the host and on the device (nothing on the host
can know it was skipped without a sync), later bias corrections see t one higher, and the parameters' version counters advance
after every step, a skipped one included.  The two options are attributes of the optimizer like track_grad_norm, not part of
param_groups or state_dict(): state dicts keep interchanging with torch.optim.Adam.

Weight EMA (csrc/optim_ema.hip; include/bmc_hip_ema.h).  Adam(..., ema_decay=D, ema_warmup=False) keeps an exponential moving
average of every parameter in state[p]["ema"], updated INSIDE the step launch: the kernel holds the new p in registers and takes
three more float32 roundings, e += w * (p - e) with w = float32(1 - decay_t), 44 bytes per element instead of 36 -- no launch, no
host work and no sync is added, p and the other state come out bit for bit as without the option, and a step that
nonfinite="skip" dropped leaves the averages untouched like everything else.  decay_t is D, or with ema_warmup min(D, t / (t + 9))
for the 1-based step count t of the bias corrections (a skipped step counts).  The average is created as a copy of p when the
parameter's state is created, or when a loaded state has none (a torch.optim.Adam state dict, a checkpoint of a run without
EMA); it travels through state_dict() / load_state_dict() and so through checkpoint.save_checkpoint / resume, and
torch.optim.Adam carries the extra key along untouched.  `with opt.ema_weights():` exchanges parameters and averages in place
(one bmc_ema_swap launch per device on entry, one on exit) for validation; opt.ema_state_dict(model) is model.state_dict() with the
averages in place of the parameters, the bare checkpoint of checkpoint.load_model_state.  Both options are attributes of the
optimizer, not part of param_groups.  Several ranks need nothing more: GradAllReducer gives every rank the same reduced gradients
and the step is deterministic, so every rank holds the same averages, bit for bit.
"""
from __future__ import annotations

import contextlib
import numbers
from collections import OrderedDict

import numpy as np
import torch

from . import ema_lib, lib
from . import ops  # noqa: F401  -- registers the global pre-step hook (ops._join_before_step) wherever this optimizer is used

CHUNK = lib.const("BMC_ADAM_CHUNK")
CHUNK_DTYPE = lib.dtype("bmc_adam_chunk_t")
STEP_LAUNCHES = 0                 # calls of bmc_adam_step / bmc_adam_step_capturable of this process
NORM_LAUNCHES = 0                 # calls of bmc_adam_grad_sq of this process (a clipped step: one per step launch)
TABLE_COPIES = 0                  # chunk tables copied to the device
MEMO_TABLES = 8                   # chunk tables kept per optimizer
_REFUSED = ("maximize", "foreach", "fused", "differentiable", "decoupled_weight_decay")


def chunk_table(entries):
    """The chunk table of one launch, a pure host function.  entries: per parameter (p, g, m, v, vmax, n) -- five addresses (vmax 0
    or None without amsgrad; g None: the parameter has no gradient and is left out) and the element count.  -> CHUNK_DTYPE array:
    a parameter of n elements gives ceil(n / 4096) consecutive chunks, none spans two parameters; `aligned` is set where all
    five addresses are multiples of 16 (a chunk starts a multiple of 16 KiB after its tensor, so it shares the tensor's alignment)."""
    rows = [(p, g, m, v, x or 0, n) for p, g, m, v, x, n in entries if g is not None]
    if not rows:
        return np.zeros(0, CHUNK_DTYPE)
    a = np.asarray(rows, dtype=np.uint64)
    if int(a[:, 5].min()) < 1:
        raise ValueError("chunk_table: a parameter without elements")
    n = a[:, 5].astype(np.int64)
    per = (n + CHUNK - 1) // CHUNK
    which = np.repeat(np.arange(len(rows)), per)
    first = np.repeat(np.cumsum(per) - per, per)
    off = (np.arange(int(per.sum())) - first) * CHUNK                      # element offset of the chunk inside its tensor
    tab = np.zeros(len(which), CHUNK_DTYPE)
    byte = (4 * off).astype(np.uint64)
    for c, key in enumerate(("p", "g", "m", "v")):
        tab[key] = a[which, c] + byte
    tab["vmax"] = np.where(a[which, 4] != 0, a[which, 4] + byte, np.uint64(0))
    tab["n"] = np.minimum(CHUNK, n[which] - off)
    tab["aligned"] = ((a[:, 0] | a[:, 1] | a[:, 2] | a[:, 3] | a[:, 4]) & np.uint64(15))[which] == 0
    return tab


def ema_chunk_table(entries):
    """The chunk table of a launch with EMA, a pure host function.  entries: per parameter (p, g, m, v, vmax, n, e), chunk_table's
    six and the address of the average.  -> (CHUNK_DTYPE array, uint64 array): the table, `aligned` cleared where the average is not
    16-byte aligned, and parallel to it the EMA pointer of every chunk, at the chunk's first element."""
    rows = [r for r in entries if r[1] is not None]
    tab = chunk_table([r[:6] for r in rows])
    if not rows:
        return tab, np.zeros(0, np.uint64)
    per = (np.asarray([r[5] for r in rows], dtype=np.int64) + CHUNK - 1) // CHUNK
    which = np.repeat(np.arange(len(rows)), per)
    p = np.asarray([r[0] for r in rows], dtype=np.uint64)[which]
    e = np.asarray([r[6] for r in rows], dtype=np.uint64)[which]
    tab["aligned"] = tab["aligned"] * ((e & np.uint64(15)) == 0)
    return tab, e + (tab["p"] - p)


def ema_decay_at(decay, warmup, t):
    """decay_t of the step whose 1-based count is t, in float64: min(decay, t / (t + 9)) with warm-up, else decay."""
    t = float(t)
    return min(float(decay), t / (t + 9.0)) if warmup else float(decay)


def ema_weight(decay, warmup, t):
    """w = float32(1 - decay_t): a float64 subtraction rounded once, the value the capturable kernels compute on the device."""
    return float(np.float32(1.0 - ema_decay_at(decay, warmup, t)))


def step_hyper(lr, beta1, beta2, eps, weight_decay, amsgrad, step):
    """bmc_adam_hyper_t of step `step` (1-based): float64 arithmetic exactly as torch's _single_tensor_adam, each value rounded
    to float32 once (by the ctypes field)."""
    h = lib.AdamHyper()
    h.lr, h.beta1_f64, h.beta2_f64 = lr, beta1, beta2
    h.beta1, h.one_minus_beta1, h.beta2, h.one_minus_beta2 = beta1, 1 - beta1, beta2, 1 - beta2
    h.eps, h.weight_decay, h.amsgrad = eps, weight_decay, int(bool(amsgrad))
    if step is not None:
        h.step_size = lr / (1 - beta1 ** step)
        h.bias_correction2_sqrt = (1 - beta2 ** step) ** 0.5
    return h


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, capturable=False,
                 track_grad_norm=False, foreach=None, maximize=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                 max_grad_norm=None, nonfinite="propagate", ema_decay=None, ema_warmup=False):
        _check_clip(max_grad_norm, nonfinite)                # before the parameters are looked at
        _check_ema(ema_decay, ema_warmup)
        if isinstance(lr, torch.Tensor):
            raise ValueError("bmc_hip.optim.Adam: a tensor lr is not supported (the step size is computed on the host)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if any(isinstance(b, torch.Tensor) for b in betas) or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # torch's group keys, all of them: a state_dict of this optimizer loads into torch.optim.Adam and back
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        _check_group(defaults)
        self.track_grad_norm = bool(track_grad_norm)
        self.max_grad_norm = max_grad_norm                   # None: never clip
        self.nonfinite = nonfinite                           # "propagate" | "skip"
        self.ema_decay = ema_decay                           # None: no weight EMA
        self.ema_warmup = ema_warmup
        self._in_ema = False                                 # inside ema_weights(): parameters and averages are exchanged
        self._ema_seen = {}                                  # parameter -> its average, once its shape, dtype and device are checked
        self._clip_memo = OrderedDict()   # the tables' keys of a clipped step -> its float64 partials (one array for all launches)
        self._clip_info = self._skipped = None               # device float64[2] {norm, c}; device int32 count of skipped steps
        self._clip_stepped = False
        self._memo = OrderedDict()        # data pointers of a launch -> (device table, chunks, partials or None)
        self._pinned = self._pinned_event = None
        self._norm_parts = None           # the partials the last step() wrote
        self._cohorts = {}                # capturable: ids of the parameters of a launch -> their device int32 step counter
        self._cohort_of = {}
        self._count = {}                  # capturable: parameter -> (its step tensor, the count the host believes it holds)
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        _check_group(group)
        for i, p in enumerate(group["params"]):
            _check_param(p, _name(group, i, len(self.param_groups) - 1))

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._cohorts.clear(); self._cohort_of.clear(); self._count.clear()       # the state tensors are other tensors now
        self._memo.clear(); self._clip_memo.clear(); self._ema_seen.clear()

    # ------------------------------------------------------------------ one step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        _check_clip(self.max_grad_norm, self.nonfinite)
        _check_ema(self.ema_decay, self.ema_warmup)
        if self._in_ema:
            raise RuntimeError("bmc_hip.optim.Adam: step() inside ema_weights(): the parameters hold the averages; leave the block first")
        if self._clipping:
            self._step_clipped()
            return loss
        parts = []
        for gi, group in enumerate(self.param_groups):
            self._step_group(gi, group, parts)
        if self.track_grad_norm:
            self._norm_parts = parts
        return loss

    @property
    def _clipping(self):
        return self.max_grad_norm is not None or self.nonfinite == "skip"

    def _step_group(self, gi, group, parts):
        amsgrad, cap = bool(group["amsgrad"]), bool(group["capturable"])
        for (dev, count), rows in self._collect(gi, group).items():
            self._launch(group, dev, count, rows, amsgrad, cap, parts)

    def _collect(self, gi, group):
        """The launches of one group: (device index, step count) -> [(p, grad, state)], state made where it is missing."""
        _check_group(group)
        amsgrad, cap = bool(group["amsgrad"]), bool(group["capturable"])
        launches = {}
        for i, p in enumerate(group["params"]):
            g = p.grad
            if g is None:
                continue
            if g.is_sparse or g.dtype != p.dtype or g.device != p.device or g.shape != p.shape or not g.is_contiguous():
                raise ValueError("bmc_hip.optim.Adam: the gradient of %s (%s, %s, %s, %s%s) does not match its parameter (%s, %s, %s): "
                                 "a dense contiguous gradient of the parameter's shape, dtype and device is required" % (
                                     _name(group, i, gi), tuple(g.shape), g.dtype, g.device, g.layout,
                                     "" if g.is_sparse or g.is_contiguous() else ", not contiguous", tuple(p.shape), p.dtype, p.device))
            st = self.state[p]
            if len(st) == 0:
                _check_param(p, _name(group, i, gi))
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if cap else torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if amsgrad:
                    st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if cap:
                    self._count[p] = (st["step"], 0)
            elif amsgrad and "max_exp_avg_sq" not in st:
                raise ValueError("bmc_hip.optim.Adam: the state of %s has no max_exp_avg_sq (amsgrad switched on after the first step)"
                                 % _name(group, i, gi))
            if self.ema_decay is not None:
                e = st.get("ema")
                if e is None or self._ema_seen.get(p) is not e:          # (a tensor is looked at once, not at every step)
                    if e is None:                            # a new state, or a loaded one without the key: the weights as they are
                        e = st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
                    elif e.dtype != p.dtype or e.device != p.device or e.shape != p.shape or not e.is_contiguous():
                        raise ValueError("bmc_hip.optim.Adam: the EMA of %s (%s, %s, %s%s) does not match its parameter: a dense "
                                         "contiguous tensor of the parameter's shape, dtype and device is required" % (
                                             _name(group, i, gi), tuple(e.shape), e.dtype, e.device, "" if e.is_contiguous() else ", not contiguous"))
                    self._ema_seen[p] = e
            step_t = st["step"]
            if cap:
                if not step_t.is_cuda:
                    step_t = st["step"] = step_t.to(device=p.device, dtype=torch.float32)
                seen = self._count.get(p)
                if seen is None or seen[0] is not step_t:
                    seen = (step_t, int(step_t.item()))      # once after load_state_dict (not inside a capture: it reads the device)
                count = seen[1]
                self._count[p] = (step_t, count + 1)
            else:
                if step_t.is_cuda:
                    step_t = st["step"] = step_t.cpu()
                count = step_t.item()
            launches.setdefault((p.device.index, count), []).append((p, g, st))
        return launches

    def _launch(self, group, dev, count, rows, amsgrad, cap, parts):
        with _current(dev):
            table, n_chunks, partial = self._table(_table_key(rows, amsgrad, self.ema_decay is not None), dev)
            self._issue(group, dev, count, rows, amsgrad, cap, table, n_chunks, partial.data_ptr() if partial is not None else None)
        if partial is not None:
            parts.append(partial)

    def _issue(self, group, dev, count, rows, amsgrad, cap, table, n_chunks, last):
        """One step launch over `table` on the current stream of `dev` (the current device).  last: the partials pointer of an
        unclipped step (None: no partials) or the AdamClip of a clipped one -- it picks the entry point."""
        global STEP_LAUNCHES
        beta1, beta2 = group["betas"]
        h = step_hyper(group["lr"], beta1, beta2, group["eps"], group["weight_decay"], amsgrad, None if cap else count + 1)
        stream = torch._C._cuda_getCurrentRawStream(dev)
        if self.ema_decay is None:
            fn, name = _ENTRY[isinstance(last, lib.AdamClip), cap]
            args = (table.data_ptr(), n_chunks, h)
        else:                                                # the same launch with the averages: the EMA pointers follow the table
            fn, name = _EMA_ENTRY[isinstance(last, lib.AdamClip), cap]
            ema = ema_lib.AdamEma()
            ema.e, ema.decay, ema.warmup = table.data_ptr() + n_chunks * CHUNK_DTYPE.itemsize, self.ema_decay, int(self.ema_warmup)
            ema.w = 0.0 if cap else ema_weight(self.ema_decay, self.ema_warmup, count + 1)
            args = (table.data_ptr(), n_chunks, h, ema)
        if cap:
            lib.call(fn, name, *args, self._cohort(rows, dev).data_ptr(), last, stream)
        else:
            lib.call(fn, name, *args, last, stream)
        # torch's own state key: host tensors (no launch), or with capturable kept true on the device; a skipped step counts too
        torch._foreach_add_([st["step"] for _, _, st in rows], 1.0)
        STEP_LAUNCHES += 1
        # the kernel wrote the parameters behind autograd's back: everything keyed on p._version must see a new version (also
        # after a skipped step)
        torch.autograd.graph.increment_version([p for p, _, _ in rows])

    def _table(self, key, dev):
        global TABLE_COPIES
        hit = self._memo.get(key)
        if hit is not None:
            self._memo.move_to_end(key)
            return hit
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("bmc_hip.optim.Adam: this set of parameter, gradient and state buffers has no chunk table on the device "
                               "yet and none can be copied during a graph capture; take one step() with the same buffers first")
        if len(key[0]) == 7:                                 # with EMA: the pointer array travels behind the table, in the same copy
            tab, eptr = ema_chunk_table(key)
            host = np.concatenate([tab.view(np.uint8).reshape(-1), eptr.view(np.uint8)])
        else:
            tab = chunk_table([k for k in key])
            host = tab.view(np.uint8).reshape(-1)
        nbytes = host.nbytes
        if self._pinned is None or self._pinned.numel() < nbytes:
            if self._pinned_event is not None:
                self._pinned_event.synchronize()
            self._pinned = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
            self._pinned_event = torch.cuda.Event()
        else:
            self._pinned_event.synchronize()                 # the copy of the previous table has read the buffer
        self._pinned[:nbytes].copy_(torch.from_numpy(host))
        table = torch.empty(nbytes, dtype=torch.uint8, device=torch.device("cuda", dev))
        table.copy_(self._pinned[:nbytes], non_blocking=True)
        self._pinned_event.record()
        TABLE_COPIES += 1
        partial = torch.empty(len(tab), dtype=torch.float64, device=table.device) if self.track_grad_norm and not self._clipping else None
        hit = self._memo[key] = (table, len(tab), partial)
        while len(self._memo) > MEMO_TABLES:
            self._memo.popitem(last=False)
        return hit

    # ------------------------------------------------------------------ one clipped step
    def _step_clipped(self):
        """k norm launches into ONE partials array, then k step launches that each read all of it (k: the launches of an
        unclipped step).  The norm is global: over every parameter that has a gradient, across groups and cohorts."""
        global NORM_LAUNCHES
        devs = {p.grad.device for group in self.param_groups for p in group["params"] if p.grad is not None}
        if len(devs) > 1:
            raise ValueError("bmc_hip.optim.Adam: the gradients of a clipped step live on %s; one global norm needs them on one "
                             "device" % ", ".join(sorted(str(d) for d in devs)))
        plan = []
        for gi, group in enumerate(self.param_groups):
            amsgrad, cap = bool(group["amsgrad"]), bool(group["capturable"])
            for (dev, count), rows in self._collect(gi, group).items():
                plan.append((group, dev, count, rows, amsgrad, cap))
        if not plan:
            return
        dev = plan[0][1]
        with _current(dev):
            keys = tuple(_table_key(rows, amsgrad, self.ema_decay is not None) for _, _, _, rows, amsgrad, _ in plan)
            tables = [self._table(key, dev) for key in keys]
            partials = self._clip_buffers(keys, sum(n for _, n, _ in tables), dev)
            stream = torch._C._cuda_getCurrentRawStream(dev)
            at = 0
            for table, n_chunks, _ in tables:                # all norm launches first ...
                lib.call(lib._adam_grad_sq, "bmc_adam_grad_sq", table.data_ptr(), n_chunks, partials.data_ptr() + 8 * at, stream)
                NORM_LAUNCHES += 1
                at += n_chunks
            for j, (launch, (table, n_chunks, _)) in enumerate(zip(plan, tables)):
                clip = lib.AdamClip()                        # ... then the step launches, each reading the whole array
                clip.partial_sq, clip.n_partials = partials.data_ptr(), partials.numel()
                clip.max_norm = float("inf") if self.max_grad_norm is None else self.max_grad_norm
                clip.skip_nonfinite = int(self.nonfinite == "skip")
                if j == 0:                                   # the first step launch of the step reports
                    clip.info, clip.skipped = self._clip_info.data_ptr(), self._skipped.data_ptr()
                self._issue(*launch, table, n_chunks, clip)
        self._norm_parts = [partials]
        self._clip_stepped = True

    def _clip_buffers(self, keys, n_partials, dev):
        """The partials array of a clipped step, memoised like the chunk tables by the buffers of all its launches; the info and
        skipped buffers live as long as the optimizer.  Nothing is allocated during a graph capture."""
        partials = self._clip_memo.get(keys)
        device = torch.device("cuda", dev)
        if partials is not None and self._clip_info is not None and self._clip_info.device == device:
            self._clip_memo.move_to_end(keys)
            return partials
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("bmc_hip.optim.Adam: this set of parameter, gradient and state buffers has no partials buffer on the "
                               "device yet and none can be allocated during a graph capture; take one step() with the same buffers first")
        if self._clip_info is None or self._clip_info.device != device:
            self._clip_info = torch.zeros(2, dtype=torch.float64, device=device)
            self._skipped = torch.zeros((), dtype=torch.int32, device=device)
        if partials is None:
            partials = self._clip_memo[keys] = torch.zeros(n_partials, dtype=torch.float64, device=device)
            while len(self._clip_memo) > MEMO_TABLES:
                self._clip_memo.popitem(last=False)
        return partials

    def last_clip(self):
        """The device float64[2] tensor {norm, c} of the last clipped step(): the global L2 norm of its gradients and the
        coefficient they were multiplied by (1.0: not clipped).  After a skipped step the norm is not finite.  No host sync."""
        if not self._clipping:
            raise RuntimeError("bmc_hip.optim.Adam: last_clip() needs max_grad_norm or nonfinite='skip'")
        if not self._clip_stepped:
            raise RuntimeError("bmc_hip.optim.Adam: last_clip() before the first step() that had gradients")
        return self._clip_info

    def skipped_steps(self):
        """A 0-d device int32 tensor: the steps skipped so far under nonfinite='skip'.  No host sync."""
        if not self._clipping:
            raise RuntimeError("bmc_hip.optim.Adam: skipped_steps() needs max_grad_norm or nonfinite='skip'")
        if not self._clip_stepped:
            raise RuntimeError("bmc_hip.optim.Adam: skipped_steps() before the first step() that had gradients")
        return self._skipped

    # ------------------------------------------------------------------ the averages
    @contextlib.contextmanager
    def ema_weights(self):
        """with opt.ema_weights(): the parameters hold their averages inside the block (validation, a "best" checkpoint) and the
        raw weights come back after it, also when the block raises.  One bmc_ema_swap launch per device on entry and one on exit
        exchange p and state[p]["ema"] in place, bit for bit; the parameters' version counters advance both times, so weight packs,
        chains, ops.bias_dense and inference graphs see the other weights.  A parameter without an average yet keeps its value.
        Not inside itself, not during a graph capture, and step() is refused inside."""
        if self.ema_decay is None:
            raise RuntimeError("bmc_hip.optim.Adam: ema_weights() needs ema_decay")
        if self._in_ema:
            raise RuntimeError("bmc_hip.optim.Adam: ema_weights() inside ema_weights(): the parameters already hold the averages")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("bmc_hip.optim.Adam: ema_weights() during a graph capture: the exchange is not part of a captured step")
        self._swap()
        self._in_ema = True
        try:
            yield self
        finally:
            self._in_ema = False
            self._swap()

    @torch.no_grad()
    def _swap(self):
        per_dev = {}
        for group in self.param_groups:
            for p in group["params"]:
                e = self.state.get(p, {}).get("ema")
                if e is not None:
                    per_dev.setdefault(p.device.index, []).append((p, e))
        for dev, pairs in per_dev.items():
            key = tuple((p.data_ptr(), 0, 0, 0, 0, p.numel(), e.data_ptr()) for p, e in pairs)      # of a chunk only p, n, aligned are read
            with _current(dev):
                table, n_chunks, _ = self._table(key, dev)
                lib.call(ema_lib._ema_swap, "bmc_ema_swap", table.data_ptr(), table.data_ptr() + n_chunks * CHUNK_DTYPE.itemsize,
                         n_chunks, torch._C._cuda_getCurrentRawStream(dev))
            torch.autograd.graph.increment_version([p for p, _ in pairs] + [e for _, e in pairs])

    def ema_state_dict(self, model):
        """model.state_dict() with every tensor that is one of this optimizer's parameters replaced by its average (a parameter
        that has none yet keeps its own value); alias keys are kept, nothing else is touched.  The bare checkpoint that
        checkpoint.load_model_state, MultiStreamSR and the reference's load_model consume.  Inside ema_weights() the parameters ARE
        the averages and the dict is model.state_dict()."""
        sd = model.state_dict()
        if self._in_ema:
            return sd
        mine = {}
        for group in self.param_groups:
            for p in group["params"]:
                e = self.state.get(p, {}).get("ema")
                if e is not None:
                    mine[(p.data_ptr(), tuple(p.shape), tuple(p.stride()))] = e.detach()
        for k, v in sd.items():
            e = mine.get((v.data_ptr(), tuple(v.shape), tuple(v.stride()))) if isinstance(v, torch.Tensor) else None
            if e is not None:
                sd[k] = e
        return sd

    def _cohort(self, rows, dev):
        """capturable: the device int32 step counter of the parameters that leave in one launch.  It is made from the first
        parameter's own `step` tensor (the device holds the truth: a replayed graph advances both without the host), and a
        parameter belongs to one cohort at a time."""
        ckey = tuple(id(p) for p, _, _ in rows)
        c = self._cohorts.get(ckey)
        if c is not None and all(self._cohort_of.get(p) == ckey for p, _, _ in rows):
            return c
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("bmc_hip.optim.Adam(capturable=True): take one step() before capturing one (the step counter of this "
                               "set of parameters is made outside a capture)")
        for p, _, _ in rows:
            self._cohorts.pop(self._cohort_of.get(p), None)
            self._cohort_of[p] = ckey
        c = self._cohorts[ckey] = rows[0][2]["step"].to(torch.int32).reshape(1).clone()
        return c

    def step_counter(self, group=0):
        """capturable: the device int32 counters (one per launch) of a group's parameters, for inspection."""
        ids = {id(p) for p in self.param_groups[group]["params"]}
        return [c for k, c in self._cohorts.items() if ids.issuperset(k)]

    # ------------------------------------------------------------------ gradient norm
    def grad_norm(self):
        """L2 norm of the raw gradients the last step() consumed (before weight decay): a 0-d float64 device tensor, the square
        root of the sum of the per-chunk float64 partials the kernel stored (with clipping on: the norm launches' partials, the
        norm BEFORE clipping).  No host sync."""
        if not (self.track_grad_norm or self._clipping):
            raise RuntimeError("bmc_hip.optim.Adam: grad_norm() needs track_grad_norm=True")
        if not self._norm_parts:
            raise RuntimeError("bmc_hip.optim.Adam: grad_norm() before the first step() that had gradients")
        parts = self._norm_parts
        flat = parts[0] if len(parts) == 1 else torch.cat([q.to(parts[0].device) for q in parts])
        return flat.sum().sqrt()


# (clipped, capturable) -> the entry point of a step launch
_ENTRY = {(False, False): (lib._adam_step, "bmc_adam_step"), (False, True): (lib._adam_step_cap, "bmc_adam_step_capturable"),
          (True, False): (lib._adam_step_clip, "bmc_adam_step_clipped"),
          (True, True): (lib._adam_step_clip_cap, "bmc_adam_step_clipped_capturable")}
_EMA_ENTRY = {(False, False): (ema_lib._adam_ema_step, "bmc_adam_ema_step"),
              (False, True): (ema_lib._adam_ema_step_cap, "bmc_adam_ema_step_capturable"),
              (True, False): (ema_lib._adam_ema_step_clip, "bmc_adam_ema_step_clipped"),
              (True, True): (ema_lib._adam_ema_step_clip_cap, "bmc_adam_ema_step_clipped_capturable")}


class _current:
    """with _current(dev): device `dev` is the current one inside the block; the one before is restored after it.  A class, not a
    generator: it sits in every step of a host-bound loop."""
    __slots__ = ("dev", "prev")

    def __init__(self, dev):
        self.dev = dev

    def __enter__(self):
        self.prev = torch.cuda.current_device()
        if self.prev != self.dev:
            torch.cuda.set_device(self.dev)

    def __exit__(self, *exc):
        if self.prev != self.dev:
            torch.cuda.set_device(self.prev)


def _table_key(rows, amsgrad, ema=False):
    if ema:                                                  # ... and the address of the average
        return tuple((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                      st["max_exp_avg_sq"].data_ptr() if amsgrad else 0, p.numel(), st["ema"].data_ptr()) for p, g, st in rows)
    return tuple((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                  st["max_exp_avg_sq"].data_ptr() if amsgrad else 0, p.numel()) for p, g, st in rows)


def _check_clip(max_grad_norm, nonfinite):
    if max_grad_norm is not None:
        if isinstance(max_grad_norm, (bool, torch.Tensor)) or not isinstance(max_grad_norm, numbers.Real):
            raise ValueError("bmc_hip.optim.Adam: max_grad_norm must be None or a positive Python number, not %r" % (max_grad_norm,))
        if not float(np.float32(max_grad_norm)) > 0:         # NaN fails too; the kernel takes it as float32
            raise ValueError("bmc_hip.optim.Adam: max_grad_norm = %r is not a positive number (in float32)" % (max_grad_norm,))
    if nonfinite not in ("propagate", "skip"):
        raise ValueError("bmc_hip.optim.Adam: nonfinite must be 'propagate' or 'skip', not %r" % (nonfinite,))


def _check_ema(ema_decay, ema_warmup):
    if ema_decay is not None:
        if isinstance(ema_decay, (bool, torch.Tensor)) or not isinstance(ema_decay, numbers.Real):
            raise ValueError("bmc_hip.optim.Adam: ema_decay must be None or a Python number in [0, 1), not %r" % (ema_decay,))
        if not 0.0 <= float(ema_decay) < 1.0:                # NaN fails too
            raise ValueError("bmc_hip.optim.Adam: ema_decay = %r is not in [0, 1)" % (ema_decay,))
    if not isinstance(ema_warmup, (bool, np.bool_)):
        raise ValueError("bmc_hip.optim.Adam: ema_warmup must be True or False, not %r" % (ema_warmup,))
    if ema_warmup and ema_decay is None:
        raise ValueError("bmc_hip.optim.Adam: ema_warmup=True needs ema_decay")


def _name(group, i, gi):
    names = group.get("param_names")
    p = group["params"][i]
    return "parameter %s#%d of group %d (shape %s)" % (repr(names[i]) + " " if names else "", i, gi, tuple(p.shape))


def _check_group(group):
    given = [k for k in _REFUSED if group.get(k)]
    if given:
        raise ValueError("bmc_hip.optim.Adam does not implement %s (there is no fallback to torch's kernels)" % ", ".join(given))
    if isinstance(group["lr"], torch.Tensor):
        raise ValueError("bmc_hip.optim.Adam: a tensor lr is not supported (the step size is computed on the host)")
    if any(isinstance(b, torch.Tensor) for b in group["betas"]):
        raise ValueError("bmc_hip.optim.Adam: tensor betas are not supported")


def _check_param(p, name):
    if not p.is_cuda:
        raise ValueError("bmc_hip.optim.Adam: %s is on %s; the step runs on the GPU only (move the model before building the optimizer)"
                         % (name, p.device))
    if p.dtype != torch.float32:
        raise ValueError("bmc_hip.optim.Adam: %s is %s; only float32 parameters are supported" % (name, p.dtype))
    if p.is_sparse or not p.is_contiguous():
        raise ValueError("bmc_hip.optim.Adam: %s is not a dense contiguous tensor" % name)
