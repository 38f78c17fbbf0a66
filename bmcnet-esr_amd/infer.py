"""Streaming single-GPU inference with the reference's semantics (infer_BMCNet.py:20-103):
the recurrent state (h, h_p, h_n, previous HR prediction) is created once and carried across calls, every call
runs one window under no_grad, and the per-window latency is measured with events on the launch stream exactly
where the reference puts its `starter/ender` pair (infer_BMCNet.py:54,66-68).

MultiStreamSR runs many recordings through one model at once (slots of one batched window); evaluate_recordings is the
reference's evaluation mode 1 on top of it.  A recording is handed over as count images (open) or as the dataset's raw event
columns with the index tables of its blocks (open_events, EventRecording), encoded window by window on the GPU.  With
emit_events the result leaves the same way: the super-resolved event stream of every window, in the dataset's column format."""
import collections
import math
import statistics

import numpy as np
import torch

from bmc_hip import slots
from bmc_hip.encodings import check_hr_noise_filter, event_block_spans, event_window_indices, filter_noise, synthesize_lr
from bmc_hip.slots import check_group_size, check_hot_filter
from infer_parts import EventStream, HotFilter, Input, KeptPredictions, Metrics, Pictures, Quality, VoxelGrids

EventRecording = collections.namedtuple("EventRecording", "lr gt lr_index gt_index lr_size gt_size", defaults=(None,) * 5)
EventRecording.__doc__ = """An event-backed recording for MultiStreamSR.open_events / evaluate_recordings: lr, gt = (xs, ys, ps)
raw dataset columns on the GPU (int16, int16, float64); lr_index, gt_index [L,2] = the event range [first, end) of every
item's LR / ground-truth frame (bmc_hip.encodings.event_window_indices); lr_size = (H, W), gt_size = (gh, gw).  A recording
without ground truth: gt = gt_index = gt_size = None."""

HREventRecording = collections.namedtuple("HREventRecording", "gt gt_ts gt_size window sliding_window threshold",
                                          defaults=(2048, 1024, None))
HREventRecording.__doc__ = """An HR-only event recording for MultiStreamSR.open_hr_events / evaluate_recordings: gt = (xs, ys, ps)
and gt_ts, its float64 timestamp column, GPU tensors of a sensor of gt_size = (gh, gw); the LR stream is synthesized at the door
(bmc_hip.encodings.downsample_events) with the session's scale and `threshold` (None = scale^2), the blocks are those of
event_window_indices(lr_ts, gt_ts, window, sliding_window, scale)."""


class StreamingSR:
    """graph=True: from the third window on, a window is ONE HIP-graph replay (the ~300 kernel launches of a window are
    captured once, input and recurrent state live in static buffers) -- at small sensor sizes the eager window is bound by
    the host's launch rate, not by the GPU.

    The tensor step() returns belongs to the caller in both modes: in graph mode it is a copy of the static prediction
    buffer (the next replay overwrites that buffer).  The captured graph is tied to the input shape and to the
    parameter values it was captured with (the packed weight images are baked into it): a different input shape raises,
    a parameter update (load_state_dict, optimizer step, in-place edit -- anything that bumps a parameter's version
    counter) makes the next step() capture afresh; edits through `.data` bypass the counters -- call reset() or
    invalidate() after them.

    state_dtype=torch.bfloat16: the recurrent FEATURE state (the n_c-channel tensors h, h_p, h_n: 3 x n_c x H x W floats per
    sequence, 66 MB at 180x240 -- what a server multiplexing many sequences through one model keeps resident per sequence) is
    carried in bf16 between windows: rounded to nearest-even when a window hands it over, widened back (exactly) when the next
    one reads it.  The previous HR prediction stays fp32 (it is the caller's output).  Contract: the reference's recurrence
    with round_bf16 applied to the three feature states between windows -- oracle/bmc_oracle.py::round_bf16, pinned by
    tests/test_gpu_r5.py::test_streaming_state_in_bf16_vs_oracle_with_state_rounding; the arithmetic inside a window is unchanged."""

    def __init__(self, model, n_c=128, scale=4, plain=False, graph=False, state_dtype=None):
        if state_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError("StreamingSR: state_dtype must be None / torch.float32 / torch.bfloat16 (got %r)" % (state_dtype,))
        self.model = model.eval()
        self.n_c, self.scale, self.plain = n_c, scale, plain
        self.use_graph = graph
        self.state_dtype = None if state_dtype is torch.float32 else state_dtype
        self.reset()

    def _pack(self, out):
        """Model outputs (feature states ..., prediction) -> the carried state: features in state_dtype, prediction fp32."""
        if self.state_dtype is None:
            return tuple(out)
        return tuple(t.to(self.state_dtype) for t in out[:-1]) + (out[-1],)

    def _unpack(self, state):
        """The carried state -> what the model reads (fp32; bf16 -> fp32 is exact)."""
        if self.state_dtype is None:
            return tuple(state)
        return tuple(t.float() for t in state[:-1]) + (state[-1],)

    def state_bytes(self):
        """Bytes of recurrent state carried for the current sequence (0 before the first window)."""
        return 0 if self.state is None else sum(t.numel() * t.element_size() for t in self.state)

    def reset(self):
        """Forget the recurrent state, the timings and the captured graph with its static buffers."""
        self.state = None
        self.times_ms = []
        self._calls = 0
        self.invalidate()

    def invalidate(self):
        """Drop the captured graph (the next graph-mode step() captures again); the recurrent state is kept."""
        if getattr(self, "_graph", None) is not None and self.state is not None:
            self.state = tuple(t.clone() for t in self._state_static)      # the state outlives the static buffers
        self._graph = self._x_static = self._state_static = self._stamp = None

    def _weights_stamp(self):
        return tuple((id(p), p._version) for p in self.model.parameters())

    def _capture(self, x):
        """Capture `state <- model(x_static, state, False)` with the state in static buffers."""
        self._x_static = x.clone()
        self._state_static = [t.clone() for t in self.state]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up on a side stream, as the capture protocol asks
            self.model(self._x_static, *self._unpack(self._state_static), False)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = self.model(self._x_static, *self._unpack(self._state_static), False)
            for dst, src in zip(self._state_static, out):
                dst.copy_(src)                              # (a bf16 static buffer: copy_ rounds to nearest-even, as _pack does)
        self._graph = g
        self._stamp = self._weights_stamp()

    @torch.no_grad()
    def step(self, x, timed=True):
        """x [B,2,T>=2,H,W] on the GPU (inp_cnt.transpose(1,2) of the reference; T = 3 with the reference's default
        SEQN, infer_BMCNet.py:147 -- only frames 0 and 1 are read, models/BMCNet.py:106-107) -> HR prediction [B,2,sH,sW]."""
        B, _, _, H, W = x.shape
        if self.state is not None and tuple(self.state[0].shape) != (B, self.n_c, H, W):
            raise RuntimeError("StreamingSR: input %s does not match the carried state %s; call reset() to start a new "
                               "sequence" % (tuple(x.shape), tuple(self.state[0].shape)))
        start = end = None
        if timed:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
        self._calls += 1
        if self.state is None:
            z = lambda c: torch.zeros(B, c, H, W, device=x.device)
            if self.plain:
                out = self.model(x, z(self.n_c), z(2 * self.scale ** 2), True)
            else:
                out = self.model(x, z(self.n_c), z(self.n_c), z(self.n_c), z(2 * self.scale ** 2), True)
            self.state = self._pack(out)
            pred = out[-1]
        elif self.use_graph and self._calls >= 3:
            if self._graph is not None and self._stamp != self._weights_stamp():
                self.invalidate()                           # the graph replays the OLD packed weights
            if self._graph is None:
                self._capture(x)
            if tuple(x.shape) != tuple(self._x_static.shape):
                raise RuntimeError("StreamingSR(graph=True): input shape %s differs from the captured %s; call reset()"
                                   % (tuple(x.shape), tuple(self._x_static.shape)))
            self._x_static.copy_(x)
            self._graph.replay()
            self.state = tuple(self._state_static)
            pred = self._state_static[-1].clone()           # the caller's own copy: the next replay rewrites the buffer
        else:
            out = self.model(x, *self._unpack(self.state), False)
            self.state = self._pack(out)
            pred = out[-1]
        if timed:
            end.record()
            end.synchronize()
            self.times_ms.append(start.elapsed_time(end))
        return pred

    @staticmethod
    @torch.no_grad()
    def esr_mse(pred, gt):
        """The evaluation metric of infer_BMCNet.py:76-84: bicubic-resize the prediction to the ground truth's size when
        they differ (:77-78; EventZoom: 124x224 vs 124x222), then the mean squared error."""
        from bmc_hip import ops
        return torch.nn.functional.mse_loss(ops.bicubic_resize(pred, gt.shape[-2:]), gt)

    @staticmethod
    @torch.no_grad()
    def bicubic_mse(inp_cnt, gt, gt_size=None):
        """The baseline metric of infer_BMCNet.py:79,85: the LR count image of the window's middle frame (inp_cnt[:, 1],
        [B,2,H,W]) bicubic-upsampled to gt_sensor_resolution (default: the ground truth's size) against the ground truth."""
        from bmc_hip import ops
        size = tuple(gt.shape[-2:]) if gt_size is None else tuple(gt_size)
        return torch.nn.functional.mse_loss(ops.bicubic_resize(inp_cnt.contiguous(), size), gt)

    def latency_ms(self, skip=1):
        """Mean per-window latency (the reference's `time` metric), ignoring the first `skip` windows."""
        t = self.times_ms[skip:] or self.times_ms
        return sum(t) / max(len(t), 1)


class SlotScheduler:
    """Which recording each of S slots carries in each window -- the host-side part of MultiStreamSR, pure Python.

    Recordings are queued with their window counts and served first come, first served.  plan() advances one window:
    a recording whose windows are all done frees its slot, free slots take the next queued recordings in slot order (their
    first window is a *reset*), and every occupied slot runs its next window."""

    def __init__(self, slots):
        if not 1 <= int(slots) <= 256:
            raise ValueError("SlotScheduler: 1 <= slots <= 256 (got %r)" % (slots,))
        self.slots = [None] * int(slots)         # per slot: [handle, next window] or None
        self.n_windows = {}
        self._queue = collections.deque()
        self._next = 0

    def add(self, n_windows):
        """Queue a recording of n_windows >= 1 windows -> its handle."""
        if int(n_windows) < 1:
            raise ValueError("SlotScheduler: a recording needs at least one window (got %r)" % (n_windows,))
        h = self._next
        self._next += 1
        self.n_windows[h] = int(n_windows)
        self._queue.append(h)
        return h

    def pending(self):
        """True while a window is left to run."""
        return bool(self._queue) or any(s is not None and s[1] < self.n_windows[s[0]] for s in self.slots)

    def plan(self):
        """Advance one window -> per slot (handle, window index, reset) or None for an empty slot; None when no window is
        left."""
        for i, s in enumerate(self.slots):
            if s is not None and s[1] >= self.n_windows[s[0]]:
                self.slots[i] = None
        fresh = set()
        for i in range(len(self.slots)):
            if self.slots[i] is None and self._queue:
                self.slots[i] = [self._queue.popleft(), 0]
                fresh.add(i)
        if all(s is None for s in self.slots):
            return None
        out = []
        for i, s in enumerate(self.slots):
            if s is None:
                out.append(None)
            else:
                out.append((s[0], s[1], i in fresh))
                s[1] += 1
        return out

    @staticmethod
    def expand(plan, K):
        """A plan of GROUPS of K slots each -> per physical slot (handle, window index, reset, member) or None: group g owns
        slots gK .. gK+K-1, member j of it (slot gK+j) runs the group's window; member 0 is the group's leader."""
        return [None if p is None else p + (j,) for p in plan for j in range(K)]


def _tensors(v):
    """Every tensor reachable in v through tuples, lists and dict values."""
    if isinstance(v, dict):
        v = tuple(v.values())
    return [v] if torch.is_tensor(v) else [t for x in v for t in _tensors(x)] if isinstance(v, (tuple, list)) else []


class MultiStreamSR:
    """Many recordings through one model at once: S slots of one batched forward pass, each carrying its own recording's
    recurrent state; a recording that ends frees its slot for the next queued one (infer_BMCNet.py mode 1, :248-295, runs
    them one after another at batch 1).  Per window: bmc_slot_stage (inputs + state, exact zeros where a recording starts),
    the model under no_grad with init=False (a zero state and a zero previous prediction give what init=True gives), then
    bmc_slot_commit (state back to the pool) -- one launch each for all slots (bmc_hip/slots.py) -- and around them the
    launches of the session's parts.

    open(frames [L,2,H,W], gts [L,2,gh,gw]) queues a recording (fp32, on the GPU; windows as oracle.infer_windows: `seqn`
    frames each, the ground truth of window i is frame i+1); step() runs one window for every active slot; run() steps to the
    end; results(handle) gives per window the time (ms, events on the launch stream around the whole window, shared by the
    slots of that window) and what the parts add.

    graph=True: from the third window on a window is ONE graph replay (everything _window() launches is captured; the slot
    table is refreshed by one small copy before it); a recording that makes a part grow invalidates the graph.  Parameter
    updates invalidate the graph as in StreamingSR.
    state_dtype=torch.bfloat16: the feature states rest in bf16 between windows, as StreamingSR(state_dtype=bf16).

    Every option is one part (infer_parts.py, where each is described), kept in self.parts in the launch order of a window:
      hot_filter=dict(...)        HotFilter        the reference's hot-pixel filter for event-backed recordings
      open / open_events          Input            frames, or raw event columns encoded window by window
      a ground truth              Metrics          esr_mse / bicubic_mse per window
      quality=True | dict(...)    Quality          esr_psnr / esr_ssim / bicubic_psnr / bicubic_ssim per window (needs a ground truth)
      keep_predictions            KeptPredictions  predictions [n_windows,2,sH,sW]
      emit_events, event_times    EventStream      the super-resolved event stream: plain, timed, or on the sensor's clock
      continuous=True             EventStream      ... every window trimmed to what no later window covers: one stream in time order
      render=(kinds...)           Pictures         the reference's event-count images
      voxel_bins=B                VoxelGrids       the voxel grid of every window's events

    self_ensemble=K (2, 4 or 8; `slots` a multiple of K): geometric self-ensemble, the "+" row of super-resolution tables.  A
    recording takes a GROUP of K adjacent slots: member j sees every frame in orientation j (bit 0 of j: flipped horizontally,
    bit 1: vertically, bit 2: polarities swapped -- K = 2: identity and h; 4: also v and hv; 8: all eight; the symmetries the
    network is trained with, EventTrainSet(augment=...)) and keeps its own recurrent state in that orientation; bmc_slot_stage
    orients the frames as it gathers them, and bmc_slot_commit turns the K predictions back, averages them (a float32 sum in
    member order, times 1/K) and writes the result over the leader's row of the model's output.  Everything downstream reads
    that row: predictions, esr_mse, sr_events / sr_ts, the "esr" picture and voxels are those of the merged prediction;
    bicubic_mse, the other pictures and hot_* are as without the option.  Nothing else changes per window -- the orientation is
    table data, one stage and one commit launch, the window of an event-backed recording encoded (and filtered) once -- but a
    window costs K slots of compute: the session runs slots / K recordings at a time.  include/bmc_hip.h "multi-stream
    inference" states the contract."""

    MAX_VOXEL_BINS, MAX_COUNT_LIMIT, MAX_COUNT_TIMED = slots.MAX_VOXEL_BINS, slots.MAX_COUNT_LIMIT, slots.MAX_COUNT_TIMED
    MAX_WINDOW_CAPACITY, MAX_ITEMS_FILTERED = slots.MAX_WINDOW_CAPACITY, slots.HOT_MAX_ITEMS
    MAX_SEQN_EVENTS, MAX_WIDTH_EVENTS = slots.MAX_SEQN, slots.MAX_ENCODE_WIDTH
    RENDER_KINDS, RENDER_TABLES, check_render = Pictures.KINDS, Pictures.TABLES, staticmethod(Pictures.check)

    def __init__(self, model, slots, n_c=128, scale=4, plain=False, graph=False, state_dtype=None, keep_predictions=False,
                 seqn=3, emit_events=False, max_count=255, event_times=None, hot_filter=None, render=None, voxel_bins=None,
                 self_ensemble=None, quality=None, continuous=False):
        self.hot_filter = check_hot_filter("MultiStreamSR: ", hot_filter)  # (the argument `slots` hides the module here)
        self.self_ensemble = check_group_size("MultiStreamSR: ", self_ensemble, int(slots))
        self.render = self.check_render("MultiStreamSR: ", render)
        self.quality = Quality.check("MultiStreamSR: ", quality)          # None, "gt" or the constant data range
        if state_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError("MultiStreamSR: state_dtype must be None / torch.float32 / torch.bfloat16 (got %r)" % (state_dtype,))
        if seqn < 2:
            raise ValueError("MultiStreamSR: seqn >= 2 (the model reads frames 0 and 1 of a window)")
        if isinstance(max_count, bool) or not isinstance(max_count, int) or not 1 <= max_count <= self.MAX_COUNT_LIMIT:
            raise ValueError("MultiStreamSR: max_count must be an integer, 1 <= max_count <= %d (got %r)"
                             % (self.MAX_COUNT_LIMIT, max_count))
        EventStream.check(emit_events, event_times, max_count, continuous)
        self.continuous = bool(continuous)
        self.voxel_bins, self.event_times = VoxelGrids.check(voxel_bins, max_count), event_times
        self._wcap = 0             # events per window the sort scratch holds (the largest window_event_capacity so far)
        self.model = model.eval()
        self.S, self.n_c, self.scale, self.plain, self.seqn = int(slots), n_c, scale, plain, int(seqn)
        self.use_graph, self.keep_predictions = graph, keep_predictions
        self.state_dtype = None if state_dtype is torch.float32 else state_dtype
        self.emit_events, self.max_count = bool(emit_events), max_count
        self.sched = SlotScheduler(self.S // (self.self_ensemble or 1))      # of groups of K slots with self_ensemble=K
        self.replays = self._calls = 0
        self._recs = {}
        self._size = None          # (H, W) of the first recording, (H, W, gh, gw) once one with ground truth has been opened
        self._steps = []           # (start, end) events per window
        self._bufs = self._graph = self._stamp = None
        self._has_events = self._has_clock = False
        self._stream = EventStream()
        on = ((HotFilter(), self.hot_filter is not None), (Input(), True), (Metrics(), True), (Quality(), self.quality is not None),
              (KeptPredictions(), keep_predictions),
              (self._stream, True), (Pictures(), self.render), (VoxelGrids(), self.voxel_bins is not None))
        self.parts = [p for p, wanted in on if wanted]     # (a part keeps no reference to the session: no cycle)

    def part(self, cls):
        return next(p for p in self.parts if type(p) is cls)

    # ---------------------------------------------------------------- recordings
    def open(self, frames, gts=None, gt_size=None, event_capacity=None, window_event_capacity=None, spans=None):
        """Queue one recording -> handle.  frames [L,2,H,W], gts [L,2,gh,gw] (fp32, on the GPU); gt_size (the reference's
        gt_sensor_resolution, the bicubic baseline's size) must be the ground truth's size.  gts=None: a recording without
        ground truth (no metrics).  event_capacity (emit_events): events the output columns hold; default 2 x scale^2 x the
        sum of `frames` (one device reduction here).  window_event_capacity (event_times): events of ONE window the sort
        scratch holds; default 2 x scale^2 x the largest sum of one frame.  spans (event_times) [L,2] float64 on the host:
        (t_first, t_last) of every frame on the sensor's clock -> sr_ts is float64 on that clock."""
        self._stream.check_capacities(self, "open", event_capacity, window_event_capacity)
        given = (frames,) if gts is None else (frames, gts)
        if frames.dim() != 4 or frames.shape[1] != 2 or any(g.dim() != 4 or tuple(g.shape[:2]) != (frames.shape[0], 2)
                                                            for g in given[1:]):
            raise ValueError("MultiStreamSR.open: frames [L,2,H,W]%s (got %s)"
                             % (" and gts [L,2,gh,gw]" * (gts is not None), ", ".join(str(tuple(g.shape)) for g in given)))
        if gts is None and gt_size is not None:
            raise ValueError("MultiStreamSR.open: gt_size without a ground truth")
        spans = self._stream.check_spans(self, "open", spans, frames.shape[0])
        if not all(g.is_cuda and g.dtype == torch.float32 for g in given):
            raise ValueError("MultiStreamSR.open: %s" % ("frames must be an fp32 GPU tensor" if gts is None else
                                                         "frames and gts must be fp32 GPU tensors"))
        L = frames.shape[0]
        if L < self.seqn:
            raise ValueError("MultiStreamSR.open: %d frames, fewer than one window of seqn = %d" % (L, self.seqn))
        H, W = frames.shape[2], frames.shape[3]
        gh, gw = (None, None) if gts is None else (gts.shape[2], gts.shape[3])
        if gt_size is not None and tuple(int(v) for v in gt_size) != (gh, gw):
            raise ValueError("MultiStreamSR.open: gt_size %s differs from the ground truth's %s" % (tuple(gt_size), (gh, gw)))
        if self.quality is not None and gts is not None:
            Quality.check_size("open", gh, gw)
        event_capacity, window_event_capacity = self._stream.room(
            self, "open", H, W, event_capacity, window_event_capacity, lambda: frames.sum(dtype=torch.float64).item(),
            lambda: frames.sum(dim=(1, 2, 3), dtype=torch.float64).max().item())
        self._set_size("open", H, W, gh, gw)
        rec = {"frames": frames.contiguous()}
        if gts is not None:
            rec["gts"] = gts.contiguous()
        return self._add(rec, L, frames.device, event_capacity, window_event_capacity, spans)

    def _set_size(self, who, H, W, gh=None, gw=None):
        """The session's size: (H, W) and, once a recording with ground truth has been opened, (gh, gw).  A recording without
        ground truth (gh None) only has to match (H, W)."""
        size = (H, W) if gh is None else (H, W, gh, gw)
        if self._size is not None and self._size[:len(size)] != size[:len(self._size)]:
            raise ValueError("MultiStreamSR.%s: sizes %s differ from the first recording's %s (group recordings by sensor "
                             "size)" % (who, size, self._size))
        if self._size is None or len(size) > len(self._size):
            if self._size is None:                         # once per session: workgroups per slot of the emit launches
                self._nparts, self._vparts = (f(self.scale * H, self.scale * W) for f in (slots.emit_parts, slots.voxel_parts))
            self._size = size
            if len(size) == 4:                             # a running session without ground truth: the metrics launch joins
                self._grow()

    def _grow(self):
        """The session gains something (a first event-backed, clocked or ground-truth recording, a larger window capacity).  One
        that has run already rebuilds the buffers whose declared shape changed and no others (the hot-pixel counts live in one),
        replaces the table when a keyword changed, and drops its captured graph, which holds the old addresses and launches."""
        b = self._bufs
        if b is None:
            return
        device = b["x"].device
        for k, d in self._scratch().items():
            if k not in b or b[k].shape != torch.Size(d[0]):
                b[k] = self._alloc(d, device)
        if any(getattr(b["table"], k) != v for k, v in self._table_keywords().items()):
            b["table"] = slots.SlotTable(self.S, device, **self._table_keywords())
        self.invalidate()

    def _add(self, rec, L, device, event_capacity=None, window_event_capacity=None, spans=None):
        """Queue a recording of L items (frames or event blocks) -> handle."""
        rec.update(n=L - self.seqn + 1, steps=[], device=device, keep=None)
        for p in self.parts:
            p.open(self, rec, L, event_capacity=event_capacity, window_event_capacity=window_event_capacity, spans=spans)
        if any([p.grew(self, rec) for p in self.parts]):
            self._grow()
        h = self.sched.add(rec["n"])
        self._recs[h] = rec
        return h

    def open_events(self, lr, gt=None, lr_index=None, gt_index=None, lr_size=None, gt_size=None, event_capacity=None,
                    window_event_capacity=None, lr_ts=None, spans=None, noise_filter=None):
        """Queue one event-backed recording -> handle.  lr, gt = (xs, ys, ps): the raw dataset columns of the LR and the
        ground-truth stream (1-D int16, int16, float64 GPU tensors; polarities -1 / 0 / +1); lr_index, gt_index [L,2]
        (integers, on the host): item j is LR events [lr_index[j,0], lr_index[j,1]) and ground-truth events [gt_index[j,0],
        gt_index[j,1]) -- bmc_hip.encodings.event_window_indices gives the reference's tables.  Window i reads the LR frames of
        items i .. i+seqn-1 and the ground truth of item i+1, as open() on the encoded frames.  Every range is checked here
        against the column lengths: the kernel trusts the table.  event_capacity (emit_events): events the output columns
        hold; default 2 x scale^2 x the sum of the lengths of the LR item ranges.  window_event_capacity (event_times): events of
        ONE window the sort scratch holds; default 2 x scale^2 x the longest LR item range.
        gt = gt_index = gt_size = None (all three or none): a recording without ground truth (no metrics).
        lr_ts (event_times): the recording's float64 timestamp column, parallel to lr[0], on the GPU or the host -> the span
        of every item (bmc_hip.encodings.event_block_spans) and float64 sr_ts on the sensor's clock; or spans [L,2] directly
        (not both).
        noise_filter=dict(ts=, dt=, support=) (bmc_hip.encodings.check_noise_filter; a session needs no event_times for it, and
        lr_ts / spans keep their own rules): the background-activity filter of include/bmc_hip_denoise.h runs ONCE, here, over the
        whole LR stream -- nothing is added to a window -- and the recording holds the LR polarity column with the dropped events
        given weight +0.0: by construction it equals open_events on (xs, ys, ps * keep).  The caller's tensors are not modified;
        lr_index, capacities and spans are untouched; the ground truth is not filtered; results() gains noise_events, the events
        dropped.  With hot_filter the hot-pixel filter observes the filtered column: a dropped event that is the last of its
        pixel in an item gives observation 0."""
        who = "MultiStreamSR.open_events: "
        self._stream.check_capacities(self, "open_events", event_capacity, window_event_capacity)
        if lr_index is None or lr_size is None:
            raise ValueError(who + "lr_index and lr_size are required")
        has_gt = gt is not None
        if (gt_index is not None) != has_gt or (gt_size is not None) != has_gt:
            raise ValueError(who + "gt, gt_index and gt_size are all given or all None")
        if lr_ts is not None and spans is not None:
            raise ValueError(who + "give lr_ts or spans, not both")
        self._stream.check_spans(self, "open_events", lr_ts if spans is None else spans)
        for name, cols in (("lr", lr), ("gt", gt))[:1 + has_gt]:
            if not (isinstance(cols, (tuple, list)) and len(cols) == 3 and all(torch.is_tensor(t) for t in cols)):
                raise ValueError(who + "%s must be three tensors (xs, ys, ps)" % name)
            if [t.dtype for t in cols] != [torch.int16, torch.int16, torch.float64]:
                raise ValueError(who + "%s columns must be int16, int16, float64 (got %s)" % (name, [t.dtype for t in cols]))
            if any(t.dim() != 1 or t.numel() != cols[0].numel() or not t.is_contiguous() for t in cols):
                raise ValueError(who + "%s columns must be contiguous 1-D tensors of one length" % name)
        tables = []
        for name, idx, n in (("lr_index", lr_index, lr[0].numel()), ("gt_index", gt_index, gt[0].numel() if has_gt else 0))[:1 + has_gt]:
            a = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx)
            if a.ndim != 2 or a.shape[1] != 2 or a.dtype.kind not in "iu":
                raise ValueError(who + "%s must be an integer [L,2] table (got %s %s)" % (name, a.dtype, a.shape))
            a = a.astype(np.int64)
            if (a[:, 0] > a[:, 1]).any():
                raise ValueError(who + "%s has a range with first > end" % name)
            if a.size and (a.min() < 0 or a.max() > n):
                raise ValueError(who + "%s has a range outside the %d events of its columns" % (name, n))
            tables.append(a)
        lr_index, gt_index = tables if has_gt else (tables[0], None)
        if has_gt and len(lr_index) != len(gt_index):
            raise ValueError(who + "lr_index has %d rows, gt_index %d" % (len(lr_index), len(gt_index)))
        L = len(lr_index)
        if L < self.seqn:
            raise ValueError(who + "%d items, fewer than one window of seqn = %d" % (L, self.seqn))
        if self.seqn > self.MAX_SEQN_EVENTS:
            raise ValueError(who + "seqn <= %d for event-backed recordings" % self.MAX_SEQN_EVENTS)
        if lr_ts is not None:
            if not ((torch.is_tensor(lr_ts) and lr_ts.dtype == torch.float64 and lr_ts.dim() == 1) or
                    (isinstance(lr_ts, np.ndarray) and lr_ts.dtype == np.float64 and lr_ts.ndim == 1)) \
                    or len(lr_ts) != lr[0].numel() or len(lr_ts) < 1:
                raise ValueError(who + "lr_ts must be a 1-D float64 column parallel to lr[0]")
            spans = event_block_spans(lr_ts, lr_index)
        spans = self._stream.check_spans(self, "open_events", spans, L)
        try:
            (H, W), (gh, gw) = (int(v) for v in lr_size), ((int(v) for v in gt_size) if has_gt else (None, None))
        except (TypeError, ValueError):
            raise ValueError(who + "lr_size = (H, W) and gt_size = (gh, gw)") from None
        if min(H, W, gh or 1, gw or 1) < 1 or max(W, gw or 1) > self.MAX_WIDTH_EVENTS:
            raise ValueError(who + "sizes must be positive and at most %d wide (got %s, %s)"
                             % (self.MAX_WIDTH_EVENTS, (H, W), (gh, gw)))
        if self.quality is not None and has_gt:
            Quality.check_size("open_events", gh, gw)
        lengths = lr_index[:, 1] - lr_index[:, 0]
        event_capacity, window_event_capacity = self._stream.room(self, "open_events", H, W, event_capacity,
                                                                  window_event_capacity, lengths.sum, lengths.max)
        cols = tuple(lr) + (tuple(gt) if has_gt else ())
        if not all(t.is_cuda and t.device == cols[0].device for t in cols):
            raise ValueError(who + "the columns must be GPU tensors on one device")
        for name, ps in (("lr", lr[2]), ("gt", gt[2] if has_gt else None))[:1 + has_gt]:
            if not bool(((ps == 1) | (ps == -1) | (ps == 0)).all()):
                raise ValueError(who + "%s polarities must be -1, 0 or +1 (counts are integers)" % name)
        dropped = None
        if noise_filter is not None:
            lr, dropped = filter_noise(who, noise_filter, tuple(lr), (H, W))
        self._set_size("open_events", H, W, gh, gw)
        rec = {"lr": tuple(lr), "lr_index": lr_index}
        if dropped is not None:
            rec["noise_events"] = dropped
        if has_gt:
            rec.update(gt=tuple(gt), gt_index=gt_index)
        return self._add(rec, L, cols[0].device, event_capacity, window_event_capacity, spans)

    def open_hr_events(self, gt, gt_ts, gt_size, window=2048, sliding_window=1024, threshold=None, dataset_length=None,
                       event_capacity=None, window_event_capacity=None, spans=None, noise_filter=None):
        """Queue one HR-ONLY event recording -> handle.  gt = (xs, ys, ps) and gt_ts, the float64 timestamp column parallel to
        them (1-D GPU tensors), of a sensor of gt_size = (gh, gw).  The LR half is synthesized here, once, on the GPU, by
        integrate-and-fire over blocks of scale x scale pixels with the session's scale (bmc_hip.encodings.downsample_events, the
        contract: include/bmc_hip_downsample.h; threshold None = scale^2); both index tables are event_window_indices(lr_ts,
        gt_ts, window, sliding_window, scale, dataset_length); the rest is open_events, with its remaining keyword arguments:
        by construction the session is bit-identical to open_events on those LR columns.  An event_times session gets the
        synthesized lr_ts unless spans are given.  noise_filter=dict(dt=, support=) needs no ts: the synthesized column is
        supplied.  One host sync (the LR event count), nothing per window; results() gains synthesized_events."""
        who = "MultiStreamSR.open_hr_events: "
        noise_filter = check_hr_noise_filter(who, noise_filter)
        lr, lr_ts, lr_size = synthesize_lr(who, gt, gt_ts, gt_size, self.scale, threshold)
        try:
            lr_index, gt_index = event_window_indices(lr_ts.cpu().numpy(), gt_ts.cpu().numpy(), window, sliding_window, self.scale,
                                                      dataset_length)
        except ValueError as e:
            raise ValueError(who + "the %d synthesized LR events: %s" % (lr_ts.numel(), e)) from None
        if noise_filter is not None:
            noise_filter = dict(noise_filter, ts=lr_ts)
        timed = self.event_times is not None and spans is None
        h = self.open_events(lr, gt, lr_index, gt_index, lr_size, gt_size, event_capacity=event_capacity,
                             window_event_capacity=window_event_capacity, lr_ts=lr_ts if timed else None, spans=spans,
                             noise_filter=noise_filter)
        self._recs[h]["synthesized_events"] = lr_ts.numel()
        return h

    def resident_bytes(self, handle):
        """Bytes the recording keeps on the GPU: every tensor of its record -- its columns (event-backed) or frames, and what the
        parts have added to it (result sums, kept predictions, output columns with their index, pictures, voxel grids, ...)."""
        return sum(t.numel() * t.element_size() for t in _tensors(self._recs[handle]))

    def scratch_bytes(self):
        """Bytes of the session's scratch: the counted entries of the parts' scratch() declarations, which _buffers() allocates
        from, at the current sizes -- so it answers before the first step(), and a part whose buffers do not exist yet (no event-
        backed recording, no window capacity) counts 0.  Not counted: x, pred, pool, feat, the table, the stream's emit_parts."""
        return sum(math.prod(shape) * dtype.itemsize for shape, dtype, _, counted in self._scratch().values() if counted)

    def results(self, handle):
        """-> dict(time=[...] per window done so far, and what the session's parts add: esr_mse, bicubic_mse (a recording with
        ground truth; with quality also esr_psnr, esr_ssim, bicubic_psnr, bicubic_ssim); hot_pixels, hot_mask (hot_filter, event-backed recordings); noise_events (a recording opened with noise_filter); predictions; images (render); voxels; sr_events,
        sr_index, sr_ts (emit_events, event_times)).  Raises RuntimeError when the windows emitted more events than the recording's
        event_capacity, or (event_times) one window more than its window_event_capacity (the message names the capacity needed)."""
        r = self._recs[handle]
        done = len(r["steps"])
        if done:
            self._steps[r["steps"][-1]][1].synchronize()
        out = {"time": [self._steps[k][0].elapsed_time(self._steps[k][1]) for k in r["steps"]]}
        for p in self.parts:
            p.results(self, out, r, done, handle)
        if "noise_events" in r:
            out["noise_events"] = r["noise_events"]
        if "synthesized_events" in r:
            out["synthesized_events"] = r["synthesized_events"]
        return out

    # ---------------------------------------------------------------- windows
    def _scratch(self):
        """{key: (shape, dtype, fill, counted)} of every part's buffers in _bufs at the current sizes ({} before a recording)."""
        return {} if self._size is None else {k: d for p in self.parts for k, d in p.scratch(self).items()}

    @staticmethod
    def _alloc(decl, device):
        shape, dtype, fill, _ = decl
        return torch.empty(shape, dtype=dtype, device=device) if fill is None else torch.full(shape, fill, dtype=dtype, device=device)

    def _table_keywords(self):
        return {k: v for p in self.parts for k, v in p.table(self).items()}

    def _buffers(self, device):
        if self._bufs is None:
            H, W = self._size[:2]
            S, nfeat = self.S, 1 if self.plain else 3
            b = {"x": torch.zeros(S, 2, self.seqn, H, W, device=device),
                 "pred": torch.zeros(S, 2, self.scale * H, self.scale * W, device=device),
                 "table": slots.SlotTable(S, device, **self._table_keywords())}
            b.update({k: self._alloc(d, device) for k, d in self._scratch().items()})
            if self.state_dtype is None:
                b["pool"] = b["feat"] = torch.zeros(nfeat, S, H, W, self.n_c, device=device)       # the model reads the pool
            else:
                b["pool"] = torch.zeros(nfeat, S, H, W, self.n_c, device=device, dtype=self.state_dtype)
                b["feat"] = torch.zeros(nfeat, S, H, W, self.n_c, device=device)
            self._bufs = b
        return self._bufs

    def _forward(self):
        b = self._bufs
        states = [t.permute(0, 3, 1, 2) for t in b["feat"]]             # channels-last [S,n_c,H,W] views, adjacent
        return self.model(b["x"], *states, b["pred"], False)

    def _window(self):
        """The input parts ([hot_update ->] [encode ->]) stage -> model -> commit, then the other parts in list order ([-> metrics]
        [-> quality] [-> emit] [-> render] [-> voxel]): what a graph replay runs."""
        b = self._bufs
        for p in self.parts:
            if p.input:
                p.launch(self, b, None)
        slots.stage(b["table"], b["x"], b["pool"], b["feat"], b["pred"])
        out = self._forward()
        cl = lambda t: t if t.permute(0, 2, 3, 1).is_contiguous() else t.contiguous(memory_format=torch.channels_last)
        pred = out[-1].contiguous()
        slots.commit(b["table"], [cl(t) for t in out[:-1]], b["pool"], pred, b["pred"])
        for p in self.parts:
            if not p.input:
                p.launch(self, b, pred)

    def _weights_stamp(self):
        return tuple((id(p), p._version) for p in self.model.parameters())

    def invalidate(self):
        """Drop the captured graph (the next graph-mode step() captures again); the slots' states are kept."""
        self._graph = self._stamp = None

    def _capture(self):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up on a side stream: the forward alone (no state change)
            self._forward()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._window()
        self._graph = g
        self._stamp = self._weights_stamp()

    def _fill(self, plan):
        """The table entries of the window `plan`, into the table's host copy."""
        t = self._bufs["table"]
        v = {"slot": t.host()}                             # host() first: it clears the copy the other views look into
        for name in ("events", "emit", "clock", "hot", "render", "voxel", "quality", "trim"):
            if getattr(t, name, False):                    # (a table without the section: no views of it)
                v[name] = getattr(t, name + "_host")()
        K = self.self_ensemble or 1                        # the plan is of groups of K slots: the parts fill the leader's entries
        for s, p in enumerate(SlotScheduler.expand(plan, K)):
            if p is None:
                continue
            h, i, reset, j = p
            if j:                                          # a member: the leader's frames, oriented; every other entry stays 0
                slots.fill_member(v["slot"], s, j)
                continue
            r = self._recs[h]
            v["slot"][s]["flags"] = slots.ACTIVE | (slots.RESET if reset else 0)
            for part in self.parts:
                part.fill(self, v, s, r, i, reset)
            if K > 1:
                slots.fill_leader(v["slot"], s, K, self.scale * self._size[1])
            r["steps"].append(len(self._steps))

    @torch.no_grad()
    def step(self):
        """Run one window for every active slot -> False when no recording had a window left."""
        plan = self.sched.plan()
        if plan is None:
            return False
        first = next(self._recs[p[0]] for p in plan if p is not None)
        self._buffers(first["device"])
        self._fill(plan)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        self._bufs["table"].upload()
        self._calls += 1
        if self.use_graph and self._calls >= 3:
            if self._graph is not None and self._stamp != self._weights_stamp():
                self.invalidate()                          # the graph replays the OLD packed weights
            if self._graph is None:
                self._capture()
            self._graph.replay()
            self.replays += 1
        else:
            self._window()
        end.record()
        self._steps.append((start, end))
        return True

    def run(self):
        """Step until every queued recording has finished."""
        while self.step():
            pass


def evaluate_recordings(model, recordings, slots, n_c=128, scale=4, plain=False, graph=False, state_dtype=None, seqn=3,
                        gt_size=None, keep_predictions=False, emit_events=False, max_count=255, event_capacity=None, event_times=None,
                        window_event_capacity=None, hot_filter=None, render=None, voxel_bins=None, self_ensemble=None, quality=None,
                        continuous=False):
    """infer_BMCNet.py mode 1 (:248-295) through MultiStreamSR: recordings = {name: (frames [L,2,H,W], gts [L,2,gh,gw])}
    (or a sequence of such pairs, named "0", "1", ...) of one sensor size; an item may also be an EventRecording (raw event
    columns + index tables, encoded window by window: MultiStreamSR.open_events).  A recording WITHOUT ground truth is
    (frames, None) or an EventRecording with gt = None.  An HREventRecording is an HR-only event recording whose LR stream is
    synthesized at the door (MultiStreamSR.open_hr_events).  -> dict(
      results = {metric: {name: value}}  per recording the mean over its windows of esr_mse, bicubic_mse (recordings with
                                         ground truth only), time (ms), and params (millions) -- infer_body's MetricTracker
                                         result (:34,:70-86),
      mean    = {metric: mean over the recordings listed}  (results_mean, :284-291; a metric no recording has is absent)[,
      predictions = {name: [n_windows,2,sH,sW]}  with keep_predictions][,
      sr_events   = {name: (xs, ys, ps, index [n_windows+1])}  with emit_events: the super-resolved event stream of every
                                         recording (MultiStreamSR(emit_events=True); event_capacity: per recording, None =
                                         the default)][,
      sr_ts       = {name: ts float32}           with event_times="linear": the events' times inside their windows, every
                                         window in time order (window_event_capacity: per recording, None = the default)][,
      images      = {name: {kind: uint8 [n_windows,h,w,3]}}  with render: the event-count images of every recording]).
    hot_filter (the EventRecording items are filtered, frame pairs are not), render (a tuple of kinds from "lr", "bicubic", "esr",
    "gt"), voxel_bins=B (the result then carries voxels = {name: float32 [n_windows,B,sH,sW]}), self_ensemble=K (2, 4, 8; slots a
    multiple of K: every recording runs in K orientations and esr_mse, predictions, sr_events, the esr image and voxels are those
    of the merged prediction), quality=True | dict(data_range=) (results and mean then carry esr_psnr, esr_ssim, bicubic_psnr and
    bicubic_ssim for the recordings with ground truth: the mean over the windows whose value is FINITE -- an exact window has an
    infinite PSNR, an empty ground-truth channel no SSIM -- and, under the key + "_nonfinite", how many windows that left out;
    mean[key] is the mean over the recordings with a finite value, mean[key + "_nonfinite"] the total of the counts):
    MultiStreamSR's options.  continuous=True (with event_times="linear"; every recording must bring its clock, which of the items above
    only an HREventRecording does): one stream in time order per recording (MultiStreamSR(continuous=True)); the result then
    carries sr_dropped = {name: [events trimmed per window]}."""
    items = list(recordings.items()) if isinstance(recordings, dict) else [(str(i), r) for i, r in enumerate(recordings)]
    ms = MultiStreamSR(model, slots, n_c=n_c, scale=scale, plain=plain, graph=graph, state_dtype=state_dtype,
                       keep_predictions=keep_predictions, seqn=seqn, emit_events=emit_events, max_count=max_count, event_times=event_times,
                       hot_filter=hot_filter, render=render, voxel_bins=voxel_bins, self_ensemble=self_ensemble, quality=quality,
                       continuous=continuous)
    handles = []
    for name, r in items:
        if isinstance(r, EventRecording):
            if gt_size is not None and r.gt_size is not None and tuple(int(v) for v in gt_size) != tuple(int(v) for v in r.gt_size):
                raise ValueError("evaluate_recordings: gt_size %s differs from recording %s's %s"
                                 % (tuple(gt_size), name, tuple(r.gt_size)))
            handles.append((name, ms.open_events(*r, event_capacity=event_capacity,
                                                 window_event_capacity=window_event_capacity)))
        elif isinstance(r, HREventRecording):
            if gt_size is not None and tuple(int(v) for v in gt_size) != tuple(int(v) for v in r.gt_size):
                raise ValueError("evaluate_recordings: gt_size %s differs from recording %s's %s"
                                 % (tuple(gt_size), name, tuple(r.gt_size)))
            handles.append((name, ms.open_hr_events(*r, event_capacity=event_capacity,
                                                    window_event_capacity=window_event_capacity)))
        else:
            handles.append((name, ms.open(r[0], r[1], gt_size if r[1] is not None else None, event_capacity=event_capacity,
                                          window_event_capacity=window_event_capacity)))
    ms.run()
    params = sum(p.numel() for p in model.parameters()) / 1e6
    breakdown = {k: {} for k in ("esr_mse", "bicubic_mse", "time", "params")}
    # results() key -> is it on; an output of that name collects it per recording (sr_events with the recording's sr_index)
    wanted = (("predictions", keep_predictions), ("sr_events", emit_events), ("sr_ts", event_times is not None),
              ("images", ms.render), ("voxels", ms.voxel_bins is not None), ("sr_dropped", ms.continuous))
    extra = {k: {} for k, on in wanted if on}
    if ms.quality is not None:
        breakdown.update({k + tail: {} for k in Quality.KEYS for tail in ("", "_nonfinite")})
    for name, h in handles:
        r = ms.results(h)
        for k in Quality.KEYS:
            if k in r:                                     # the mean of the finite windows, and how many were not
                finite = [v for v in r[k] if math.isfinite(v)]
                breakdown[k][name] = float(statistics.mean(finite)) if finite else float("nan")
                breakdown[k + "_nonfinite"][name] = len(r[k]) - len(finite)
        for k in ("esr_mse", "bicubic_mse", "time"):
            if k in r:
                breakdown[k][name] = float(statistics.mean(r[k]))
        breakdown["params"][name] = params
        for k in extra:
            extra[k][name] = r[k] + (r["sr_index"],) if k == "sr_events" else r[k]
    mean = {k: float(statistics.mean(v.values())) for k, v in breakdown.items() if v}
    for k in Quality.KEYS:
        if breakdown.get(k):                               # recordings without a finite window are left out, the counts add up
            finite = [v for v in breakdown[k].values() if math.isfinite(v)]
            mean[k] = float(statistics.mean(finite)) if finite else float("nan")
            mean[k + "_nonfinite"] = int(sum(breakdown[k + "_nonfinite"].values()))
    return {"results": breakdown, "mean": mean, **extra}

