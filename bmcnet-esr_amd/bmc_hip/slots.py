"""Recording slots of multi-stream inference (csrc/slots.hip; include/bmc_hip.h "multi-stream inference"): the per-window
stage / commit / metrics launches of infer.MultiStreamSR, ONE launch each for all S slots.

A slot table is S bmc_slot_t entries (SLOT_DTYPE) in a device uint8 tensor; the host fills a numpy view of a pinned copy
(SlotTable) and uploads it with one small copy per window.  Feature states are laid out [nfeat][S][H][W][n_c]: the model's
channels-last [S,n_c,H,W] views of state k are `to_nchw(buf[k])`, adjacent in one buffer (ops.stack_states reads them
without a copy).  LAUNCHES counts the launches of each wrapper (the tests check that a window costs one of each).

Self-ensemble (include/bmc_hip.h "multi-stream inference" states the contract): a group of K adjacent slots carries one recording
in K orientations -- fill_leader() / fill_member() write the group's entries (ORIENT_* / GROUP_SHIFT name the bits of `flags`);
stage() then orients each member's frames, commit() merges the K predictions into the leader's row of the model's output.

Event-backed slots (csrc/slot_events.hip): a second table of S bmc_slot_events_t entries (SLOT_EVENTS_DTYPE) behind the slot
table in the same device tensor and the same pinned upload (SlotTable(events=True)); encode() builds the count images of
every slot with an event entry in one launch, counted in ENCODE_LAUNCHES.

Event output (csrc/slot_emit.hip): a third table of S bmc_slot_emit_t entries (SLOT_EMIT_DTYPE) behind the other two, same
upload (SlotTable(emit=True)); emit() turns the predictions of every slot with an emit entry into events appended to the
entry's columns (one call = two launches for all slots, counted in EMIT_LAUNCHES).

Timed event output (csrc/slot_emit_timed.hip): SlotTable(emit=True, timed=True) holds bmc_slot_emit_timed_t entries
(SLOT_EMIT_TIMED_DTYPE: the same fields and a `ts` column) instead; emit_timed() appends every window's events with their
float32 times, in time order (one call = EMIT_TIMED_KERNELS launches for all slots, counted in EMIT_TIMED_LAUNCHES).

Clocked event output: SlotTable(emit=True, timed=True, clock=True) adds a fourth table of bmc_slot_clock_t entries
(SLOT_CLOCK_DTYPE: the window's time span on the recording's clock and a float64 `ts` column); emit_clocked() is emit_timed()
whose slots with a clock entry store float64 times on that clock instead (the same launches, the same counter).

Continuous event output (csrc/slot_emit_trimmed.hip; include/bmc_hip_stream.h states the contract): SlotTable(emit=True,
timed=True, clock=True, trim=True) adds a table of bmc_slot_trim_t entries (SLOT_TRIM_DTYPE: the window's cut and where its
dropped count goes) as the LAST section; emit_trimmed() is emit_clocked() that emits only a window's events before its cut,
trimmed before the sort (the same launches, the same counter).

Hot-pixel filter (csrc/slot_hot.hip; include/bmc_hip.h "hot-pixel filter" states the contract): SlotTable(events=True, hot=True)
adds a table of bmc_slot_hot_t entries (SLOT_HOT_DTYPE) behind the others; hot_update() folds the newly observed items of every
filtered slot into its counts and writes their masks into the slot's ring (one call = HOT_KERNELS launch for all slots, counted in
HOT_LAUNCHES), encode_filtered() is encode() storing the LR frames through those masks (counted in ENCODE_LAUNCHES).

Event-count images (csrc/slot_render.hip; include/bmc_hip.h "event-count images" states the contract): SlotTable(render=K) adds K
tables of bmc_slot_render_t entries (SLOT_RENDER_DTYPE: a count image and where its picture goes) behind the others, one per kind
of image; render() draws table k's images for all slots (one call = RENDER_KERNELS launches, counted in RENDER_LAUNCHES).

Voxel grids (csrc/slot_voxel.hip; include/bmc_hip.h "voxel grids" states the contract): SlotTable(voxel=True) adds a table of
bmc_slot_voxel_t entries (SLOT_VOXEL_DTYPE: where the slot's grid goes) behind the others; voxel() turns the predictions of every
slot with a voxel entry into the temporal-bilinear voxel grid of its timed event stream, per pixel (one call = VOXEL_KERNELS
launches, counted in VOXEL_LAUNCHES).

PSNR and SSIM (csrc/slot_quality.hip; include/bmc_hip_quality.h states the contract): SlotTable(quality=True) adds a table of
bmc_slot_quality_t entries (SLOT_QUALITY_DTYPE: where the slot's raw record goes) behind the others; quality() writes, for every
slot with a quality entry, the record of the prediction and of the bicubic baseline against the slot's ground truth (one call =
QUALITY_KERNELS launches, counted in QUALITY_LAUNCHES); quality_values() finishes records into PSNR and SSIM on the host."""
import numpy as np
import torch

from . import lib, quality_lib, stream_lib
from .ops import _stream

# the header's limits and table layouts (include/bmc_hip.h), as the library states them
ACTIVE, RESET = lib.const("BMC_SLOT_ACTIVE"), lib.const("BMC_SLOT_RESET")
MAX_SLOTS = lib.const("BMC_MAX_SLOTS")
MAX_PARTS = lib.const("BMC_SLOT_MAX_PARTS")
SLOT_DTYPE = lib.dtype("bmc_slot_t")
LAUNCHES = {"stage": 0, "commit": 0, "metrics": 0}
# self-ensemble (include/bmc_hip.h "multi-stream inference"): bits of bmc_slot_t.flags that no #define carries -- the
# orientation code o (ORIENT_H | ORIENT_V | ORIENT_P, the order of the sequence encoder's `flips` bits 0..2) in bits 2..4, the
# group size K at a group's leader in bits 8..11; the leader's pad_ holds the prediction's row length sW
ORIENT_SHIFT, ORIENT_H, ORIENT_V, ORIENT_P = 2, 1, 2, 4
GROUP_SHIFT = 8
GROUP_SIZES = (2, 4, 8)
MAX_SEQN = lib.const("BMC_SLOT_MAX_SEQN")
MAX_ENCODE_WIDTH = 7680
SLOT_EVENTS_DTYPE = lib.dtype("bmc_slot_events_t")
ENCODE_LAUNCHES = 0
MAX_EMIT_PARTS = lib.const("BMC_SLOT_EMIT_MAX_PARTS")
MAX_COUNT_LIMIT = 32767            # counts and coordinates of emitted events fit int16
SLOT_EMIT_DTYPE = lib.dtype("bmc_slot_emit_t")
EMIT_LAUNCHES = 0
SLOT_EMIT_TIMED_DTYPE = lib.dtype("bmc_slot_emit_timed_t")
EMIT_TIMED_LAUNCHES = 0
EMIT_TIMED_KERNELS = 6             # launches of one bmc_slot_emit_timed call: count, scan, expand, histogram, scan, scatter
MAX_COUNT_TIMED = lib.const("BMC_SLOT_EMIT_TIMED_MAX_COUNT")       # the rank table of the timed mode
MAX_WINDOW_CAPACITY = lib.const("BMC_SLOT_EMIT_TIMED_MAX_WINDOW")
EVENT_T0, EVENT_T1 = lib.const("BMC_EVENT_T0"), lib.const("BMC_EVENT_T1")      # the window's time axis
SLOT_CLOCK_DTYPE = lib.dtype("bmc_slot_clock_t")
SLOT_TRIM_DTYPE = stream_lib.dtype("bmc_slot_trim_t")
_RANK_TABLES = {}
SLOT_HOT_DTYPE = lib.dtype("bmc_slot_hot_t")
HOT_LAUNCHES = 0
HOT_KERNELS = 1                    # launches of one bmc_slot_hot_update call
HOT_MAX_ITEMS = 1 << 23            # below it distinct counts give distinct float32 rates (the contract's rule 3)
SLOT_RENDER_DTYPE = lib.dtype("bmc_slot_render_t")
RENDER_LAUNCHES = 0
RENDER_KERNELS = 2                 # launches of one bmc_slot_render call: select, colour
MAX_RENDER_PIXELS = lib.const("BMC_SLOT_RENDER_MAX_PIXELS")        # h * w - 1 is exact in float32
MAX_RENDER_PARTS = lib.const("BMC_SLOT_RENDER_MAX_PARTS")
MAX_RENDER_TABLES = 8
SLOT_VOXEL_DTYPE = lib.dtype("bmc_slot_voxel_t")
VOXEL_LAUNCHES = 0
VOXEL_KERNELS = 2                  # launches of one bmc_slot_voxel call: reduce, voxel
MAX_VOXEL_BINS = lib.const("BMC_SLOT_VOXEL_MAX_BINS")
SLOT_QUALITY_DTYPE = quality_lib.dtype("bmc_slot_quality_t")
QUALITY_LAUNCHES = 0
QUALITY_KERNELS = 3                # launches of one bmc_slot_quality call: stats, ssim, finish
QUALITY_WIN, QUALITY_WORDS = quality_lib.const("BMC_QUALITY_WIN"), quality_lib.const("BMC_QUALITY_WORDS")
QUALITY_TILE_H, QUALITY_TILE_W = quality_lib.const("BMC_QUALITY_TILE_H"), quality_lib.const("BMC_QUALITY_TILE_W")
QUALITY_STATS_WORDS = quality_lib.const("BMC_QUALITY_STATS_WORDS")


def table_layout(S, events=False, emit=False, timed=False, clock=False, hot=False, render=0, voxel=False, quality=False,
                 trim=False):
    """The sections of a slot table of S slots -> ([(name, dtype, byte offset), ...] in their order in memory, total bytes):
    "slot" (bmc_slot_t) always, then "events", "emit" (bmc_slot_emit_timed_t entries with timed=True), "clock" (needs timed) and
    "hot" (needs events), each S entries behind the one before, "render" (render tables of S entries each), "voxel"
    (voxel=True or False: S bmc_slot_voxel_t entries), "quality" (quality=True or False: S bmc_slot_quality_t entries) and "trim"
    (needs clock: S bmc_slot_trim_t entries) -- the last section, so every other one lies where it lies without it."""
    if timed and not emit:
        raise ValueError("slots: timed=True needs emit=True")
    if clock and not timed:
        raise ValueError("slots: clock=True needs timed=True")
    if hot and not events:
        raise ValueError("slots: hot=True needs events=True")
    if trim and not clock:
        raise ValueError("slots: trim=True needs clock=True")
    if isinstance(render, bool) or not isinstance(render, int) or not 0 <= render <= MAX_RENDER_TABLES:
        raise ValueError("slots: render must be a number of tables, 0 .. %d (got %r)" % (MAX_RENDER_TABLES, render))
    if not isinstance(voxel, (bool, np.bool_)):
        raise ValueError("slots: voxel must be True or False (got %r)" % (voxel,))
    if not isinstance(quality, (bool, np.bool_)):
        raise ValueError("slots: quality must be True or False (got %r)" % (quality,))
    sections, nbytes = [], 0
    for name, dtype, count in (("slot", SLOT_DTYPE, 1), ("events", SLOT_EVENTS_DTYPE, int(bool(events))),
                               ("emit", SLOT_EMIT_TIMED_DTYPE if timed else SLOT_EMIT_DTYPE, int(bool(emit))),
                               ("clock", SLOT_CLOCK_DTYPE, int(bool(clock))), ("hot", SLOT_HOT_DTYPE, int(bool(hot))),
                               ("render", SLOT_RENDER_DTYPE, render), ("voxel", SLOT_VOXEL_DTYPE, int(voxel)),
                               ("quality", SLOT_QUALITY_DTYPE, int(quality)), ("trim", SLOT_TRIM_DTYPE, int(bool(trim)))):
        if count:
            sections.append((name, dtype, nbytes))
            nbytes += count * S * dtype.itemsize
    return sections, nbytes


class SlotTable:
    """A device slot table and a small ring of pinned host copies: `host()` returns the numpy entries to fill for the next
    window (cleared), `upload()` copies them to the device on the current stream.  A ring buffer is rewritten only after the
    copy that last read it has completed, so the host never waits for the GPU to finish the window before.
    The other sections of table_layout() share the tensor and the copy: `events_host()` / `events_ptr()` (events=True),
    `emit_host()` / `emit_ptr()` (emit=True; timed=True: bmc_slot_emit_timed_t entries), `clock_host()` / `clock_ptr()`
    (clock=True, needs timed), `hot_host()` / `hot_ptr()` (hot=True, needs events), `render_host()` [K,S] / `render_ptr(k)`
    (render=K tables), `voxel_host()` / `voxel_ptr()` (voxel=True), `quality_host()` / `quality_ptr()` (quality=True), `trim_host()` / `trim_ptr()` (trim=True, needs clock).  The *_host() views are those of the window being filled, after host(), which cleared them."""

    RING = 4

    def __init__(self, S, device, events=False, emit=False, timed=False, clock=False, hot=False, render=0, voxel=False,
                 quality=False, trim=False):
        if not 1 <= S <= MAX_SLOTS:
            raise ValueError("slots: 1 <= S <= %d (got %d)" % (MAX_SLOTS, S))
        self.S = S
        self.events, self.emit, self.timed, self.clock, self.hot = bool(events), bool(emit), bool(timed), bool(clock), bool(hot)
        self.render = render
        sections, nbytes = table_layout(S, self.events, self.emit, self.timed, self.clock, self.hot, render, voxel, quality, trim)
        self.voxel, self.quality, self.trim = bool(voxel), bool(quality), bool(trim)
        self._at = {name: (dtype, off) for name, dtype, off in sections}
        self.dev = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self._pinned = [torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(self.RING)]
        self._events = [None] * self.RING
        self._k = 0

    def _host(self, name):
        dtype, off = self._at[name]
        return self._pinned[self._k].numpy()[off:off + self.S * dtype.itemsize].view(dtype)

    def _ptr(self, name):
        return self.dev.data_ptr() + self._at[name][1]

    def host(self):
        k = self._k
        if self._events[k] is not None:
            self._events[k].synchronize()
        self._pinned[k].numpy()[:] = 0
        return self._host("slot")

    def events_host(self):
        return self._host("events")

    def emit_host(self):
        return self._host("emit")

    def clock_host(self):
        return self._host("clock")

    def hot_host(self):
        return self._host("hot")

    def render_host(self):
        dtype, off = self._at["render"]
        return self._pinned[self._k].numpy()[off:off + self.render * self.S * dtype.itemsize].view(dtype).reshape(self.render, self.S)

    def voxel_host(self):
        return self._host("voxel")

    def quality_host(self):
        return self._host("quality")

    def trim_host(self):
        return self._host("trim")

    def upload(self):
        k = self._k
        self.dev.copy_(self._pinned[k], non_blocking=True)
        ev = self._events[k] = self._events[k] or torch.cuda.Event()
        ev.record()
        self._k = (k + 1) % self.RING

    def ptr(self):
        return self._ptr("slot")

    def events_ptr(self):
        return self._ptr("events")

    def emit_ptr(self):
        return self._ptr("emit")

    def clock_ptr(self):
        return self._ptr("clock")

    def hot_ptr(self):
        return self._ptr("hot")

    def render_ptr(self, k):
        if not 0 <= k < self.render:
            raise ValueError("slots: the table has %d render tables (got %r)" % (self.render, k))
        return self._ptr("render") + k * self.S * SLOT_RENDER_DTYPE.itemsize


    def voxel_ptr(self):
        return self._ptr("voxel")

    def quality_ptr(self):
        return self._ptr("quality")

    def trim_ptr(self):
        return self._ptr("trim")


def _check(cond, what):
    if not cond:
        raise ValueError("slots: " + what)


def check_group_size(who, K, S):
    """self_ensemble K (None, or 2 / 4 / 8 dividing the S slots) -> None or K; ValueError otherwise."""
    if K is None:
        return None
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K not in GROUP_SIZES:
        raise ValueError(who + "self_ensemble must be None, 2, 4 or 8 (got %r)" % (K,))
    if S % K:
        raise ValueError(who + "slots must be a multiple of self_ensemble (got %d slots for groups of %d)" % (S, K))
    return int(K)


def fill_leader(entries, s, K, sW):
    """entries (SLOT_DTYPE, a table's host view): the filled entry s becomes the leader of the ensemble group s .. s+K-1, the
    identity member -- it gains the group size K and pad_ = sW, the prediction's row length."""
    entries[s]["flags"] = int(entries[s]["flags"]) | (K << GROUP_SHIFT)
    entries[s]["pad_"] = sW


def fill_member(entries, s, j):
    """Entry s = member j >= 1 of the group led by entry s - j: the leader's frames in orientation j, with the leader's ACTIVE /
    RESET bits, and nothing else -- no ground truth, keep or result (the kernels after commit skip the slot)."""
    lead, e = entries[s - j], entries[s]
    e["frames"], e["gt"], e["keep"], e["result"], e["pad_"] = lead["frames"], 0, 0, 0, 0
    e["flags"] = (int(lead["flags"]) & (ACTIVE | RESET)) | (j << ORIENT_SHIFT)


def _feat_layout(pool):
    """pool [nfeat, S, H, W, n_c] contiguous -> (nfeat, feat_n)."""
    _check(pool.dim() == 5 and pool.is_contiguous() and pool.dtype in (torch.float32, torch.bfloat16),
           "feature pool must be a contiguous [nfeat,S,H,W,n_c] fp32 / bf16 tensor")
    return pool.shape[0], pool.shape[2] * pool.shape[3] * pool.shape[4]


def stage(table, x, pool, feat, pred):
    """x [S,2,seqn,H,W] <- the slots' windows; feat [nfeat,S,H,W,n_c] fp32 <- the pool's state (zeros for reset / empty
    slots; feat may BE an fp32 pool); pred [S,2,sH,sW] (the previous predictions, in place) zeroed for reset / empty slots.
    A slot whose flags carry an orientation code gets its frames in that orientation."""
    S, two, seqn, H, W = x.shape
    nfeat, feat_n = _feat_layout(pool)
    _check(two == 2 and x.is_contiguous() and x.dtype == torch.float32, "x must be a contiguous fp32 [S,2,seqn,H,W]")
    _check(tuple(feat.shape) == tuple(pool.shape) and feat.dtype == torch.float32 and feat.is_contiguous(),
           "feat must be a contiguous fp32 tensor of the pool's shape")
    _check(tuple(pool.shape[1:4]) == (S, H, W) and table.S == S, "pool / table do not match x")
    _check(pred.shape[0] == S and pred.is_contiguous() and pred.dtype == torch.float32, "pred must be contiguous fp32 [S,...]")
    lib.call(lib._slot_stage, "bmc_slot_stage", table.ptr(), S, seqn, H, W, x.data_ptr(), pool.data_ptr(),
             int(pool.dtype == torch.bfloat16), feat.data_ptr(), nfeat, feat_n, pred.data_ptr(), pred[0].numel(), _stream())
    LAUNCHES["stage"] += 1


def commit(table, srcs, pool, pred_src, pred_pool):
    """Active slots: pool[k] <- srcs[k] (the model's new [S,n_c,H,W] channels-last states; bf16 pool: nearest-even),
    pred_pool <- pred_src, and the prediction to each slot's `keep` address.  The leader of an ensemble group (fill_leader):
    its row of pred_src and its `keep` then receive the group's merged prediction -- pred_src is written in place."""
    nfeat, feat_n = _feat_layout(pool)
    S = pool.shape[1]
    _check(len(srcs) == nfeat, "%d state tensors for a pool of %d" % (len(srcs), nfeat))
    ptrs = (lib.C.c_void_p * 3)()
    for k, t in enumerate(srcs):
        _check(t.dtype == torch.float32 and t.shape[0] == S and t[0].numel() == feat_n and t.permute(0, 2, 3, 1).is_contiguous(),
               "state %d must be a channels-last fp32 [S,n_c,H,W] tensor" % k)
        ptrs[k] = t.data_ptr()
    for t in (pred_src, pred_pool):
        _check(t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(pred_pool.shape),
               "predictions must be contiguous fp32 tensors of one shape")
    lib.call(lib._slot_commit, "bmc_slot_commit", table.ptr(), S, ptrs, nfeat, feat_n, pool.data_ptr(),
             int(pool.dtype == torch.bfloat16), pred_src.data_ptr(), pred_pool.data_ptr(), pred_pool[0].numel(), _stream())
    LAUNCHES["commit"] += 1


def metric_parts(gh, gw):
    """Workgroups per slot of bmc_slot_metrics for a gh x gw ground truth (about 16 elements per lane, at most 64)."""
    return max(1, min(MAX_PARTS, -(-2 * gh * gw // (1024 * 16))))


def sum_parts(sse):
    """[..., nparts, 2] partial sums (float64, any device) -> [..., 2] on the CPU, added in part order."""
    sse = sse.cpu()
    out = sse[..., 0, :].clone()
    for p in range(1, sse.shape[-2]):
        out += sse[..., p, :]
    return out


def metrics(table, pred, H, W, gh, gw, nparts):
    """Per active slot with a result address: nparts x {esr_sse, bicubic_sse} partial sums (float64) of
    sum (bicubic(pred -> gh x gw) - gt)^2 and sum (bicubic(frame 1 -> gh x gw) - gt)^2 -- the sums of infer_BMCNet.py:76-85
    (sum_parts adds them; divide by 2*gh*gw for the MSE)."""
    S, two, sH, sW = pred.shape
    _check(two == 2 and pred.is_contiguous() and pred.dtype == torch.float32 and table.S == S,
           "pred must be a contiguous fp32 [S,2,sH,sW]")
    _check(1 <= nparts <= MAX_PARTS, "1 <= nparts <= %d" % MAX_PARTS)
    lib.call(lib._slot_metrics, "bmc_slot_metrics", table.ptr(), S, pred.data_ptr(), sH, sW, H, W, gh, gw, nparts, _stream())
    LAUNCHES["metrics"] += 1


def _check_encode_args(table, lr_scratch, gt_scratch):
    """The scratch images of encode() / encode_filtered() -> (S, seqn, H, W, gh, gw)."""
    for t in (lr_scratch, gt_scratch):
        _check(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == table.S,
               "scratch must be contiguous fp32 GPU tensors [S,...]")
    _check(lr_scratch.dim() == 5 and lr_scratch.shape[2] == 2 and gt_scratch.dim() == 4 and gt_scratch.shape[1] == 2,
           "lr_scratch [S,seqn,2,H,W] and gt_scratch [S,2,gh,gw]")
    S, seqn, _, H, W = lr_scratch.shape
    gh, gw = gt_scratch.shape[2:]
    _check(2 <= seqn <= MAX_SEQN, "2 <= seqn <= %d" % MAX_SEQN)
    _check(max(W, gw) <= MAX_ENCODE_WIDTH, "frames wider than %d pixels are not supported" % MAX_ENCODE_WIDTH)
    return S, seqn, H, W, gh, gw


def encode(table, lr_scratch, gt_scratch):
    """Every slot with an event entry: lr_scratch[s] [seqn,2,H,W] and gt_scratch[s] [2,gh,gw] <- the count images of the
    entry's event ranges (bmc_slot_encode: one launch, integer counts, deterministic); other slots' scratch is not touched."""
    global ENCODE_LAUNCHES
    _check(table.events, "the slot table has no event entries (SlotTable(events=True))")
    S, seqn, H, W, gh, gw = _check_encode_args(table, lr_scratch, gt_scratch)
    lib.call(lib._slot_encode, "bmc_slot_encode", table.events_ptr(), S, seqn, H, W, gh, gw, lr_scratch.data_ptr(),
             gt_scratch.data_ptr(), _stream())
    ENCODE_LAUNCHES += 1


def check_hot_filter(who, hot_filter):
    """hot_filter (None, or a dict with exactly the keys max_px, min_obvs, max_rate) -> None or (max_px, min_obvs, max_rate);
    ValueError naming the bad key."""
    if hot_filter is None:
        return None
    keys = ("max_px", "min_obvs", "max_rate")
    if not isinstance(hot_filter, dict):
        raise ValueError(who + "hot_filter must be None or a dict with the keys %s (got %r)" % (", ".join(keys), hot_filter))
    for k in hot_filter:
        if k not in keys:
            raise ValueError(who + "hot_filter has an unknown key %r (the keys are %s)" % (k, ", ".join(keys)))
    for k in keys:
        if k not in hot_filter:
            raise ValueError(who + "hot_filter lacks the key %r" % k)
    for k in keys[:2]:
        v = hot_filter[k]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < 2 ** 31:
            raise ValueError(who + "hot_filter[%r] must be an integer, 0 <= %s < 2^31 (got %r)" % (k, k, v))
    r = hot_filter["max_rate"]
    if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or not np.isfinite(np.float32(r)):
        raise ValueError(who + "hot_filter['max_rate'] must be a finite number (got %r)" % (r,))
    return int(hot_filter["max_px"]), int(hot_filter["min_obvs"]), float(r)


def hot_cmin(idx, min_obvs, max_rate):
    """Rule 3 of the hot-pixel contract for an item with idx observations, as the integer the kernel compares counts with:
    0 (the item masks nothing) for idx <= min_obvs; 1 for max_rate < 0 (the pixels with a count; bmc_slot_hot_update's
    negative_rate adds the rule's one further pixel); else the smallest c in [0, idx] with float32(c) / float32(idx) >
    float32(max_rate), idx + 1 if there is none.  The comparison is made in float32, as torch makes it."""
    idx = int(idx)
    _check(1 <= idx < HOT_MAX_ITEMS, "1 <= idx < 2^23 (got %d)" % idx)
    if idx <= min_obvs:
        return 0
    rate = np.float32(max_rate)
    if rate < 0:
        return 1
    above = lambda c: bool(np.float32(c) / np.float32(idx) > rate)
    c = min(max(int(np.floor(float(rate) * idx)) - 2, 0), idx)        # the rounded quotient is monotone in c: search near rate * idx
    while c > 0 and above(c):
        c -= 1
    while c <= idx and not above(c):
        c += 1
    return c


def hot_update(table, counts, ring, ws, max_px, max_rate):
    """Every slot with an active hot entry (SlotTable.hot_host), for each of its window's newly observed frames in order: the
    last-writer observation of the frame's LR events, counts[s] [H,W] int32 += it (= it at a reset), the selection of the
    contract's rule 3 with the entry's cmin (hot_cmin) and max_px, the item's mask (uint8, 1 = keep) into ring[s, item % seqn];
    the last item's mask count / mask go to the entry's hot_pixels / hot_mask addresses.  ws: int32 [S,H,W] of workspace.
    One launch for all slots (bmc_slot_hot_update); inactive slots are not touched."""
    global HOT_LAUNCHES
    _check(table.events and table.hot, "the slot table has no hot entries (SlotTable(events=True, hot=True))")
    _check(torch.is_tensor(ring) and ring.dim() == 4 and ring.is_cuda and ring.is_contiguous() and ring.dtype == torch.uint8
           and ring.shape[0] == table.S, "ring must be a contiguous uint8 GPU tensor [S,seqn,H,W]")
    S, seqn, H, W = ring.shape
    for name, t in (("counts", counts), ("ws", ws)):
        _check(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and tuple(t.shape) == (S, H, W),
               "%s must be a contiguous int32 GPU tensor [S,H,W]" % name)
    _check(2 <= seqn <= MAX_SEQN, "2 <= seqn <= %d" % MAX_SEQN)
    _check(not isinstance(max_px, bool) and isinstance(max_px, (int, np.integer)) and 0 <= max_px < 2 ** 31,
           "max_px must be an integer, 0 <= max_px < 2^31 (got %r)" % (max_px,))
    lib.call(lib._slot_hot_update, "bmc_slot_hot_update", table.hot_ptr(), table.events_ptr(), S, seqn, H, W, int(max_px),
             int(np.float32(max_rate) < 0), counts.data_ptr(), ring.data_ptr(), ws.data_ptr(), _stream())
    HOT_LAUNCHES += 1


def encode_filtered(table, lr_scratch, gt_scratch, ring):
    """encode() of a filtered session (bmc_slot_encode_filtered: one launch): the LR frames of a slot with an active hot entry
    are stored through their items' masks in ring [S,seqn,H,W] (the contract's rule 4); everything else as encode()."""
    global ENCODE_LAUNCHES
    _check(table.events and table.hot, "the slot table has no hot entries (SlotTable(events=True, hot=True))")
    S, seqn, H, W, gh, gw = _check_encode_args(table, lr_scratch, gt_scratch)
    _check(torch.is_tensor(ring) and ring.is_cuda and ring.is_contiguous() and ring.dtype == torch.uint8
           and tuple(ring.shape) == (S, seqn, H, W), "ring must be a contiguous uint8 GPU tensor [S,seqn,H,W]")
    lib.call(lib._slot_encode_filtered, "bmc_slot_encode_filtered", table.events_ptr(), table.hot_ptr(), ring.data_ptr(), S, seqn,
             H, W, gh, gw, lr_scratch.data_ptr(), gt_scratch.data_ptr(), _stream())
    ENCODE_LAUNCHES += 1


def render_parts(h, w):
    """Workgroups per slot of bmc_slot_render's colour launch for an h x w image (about 4 096 pixels each, at most 1 024)."""
    return max(1, min(MAX_RENDER_PARTS, -(-h * w // 4096)))


def render(table, k, h, w, round, scratch):
    """Every active slot whose entry in render table k has a src and a dst: dst (uint8 [h,w,3]) <- the picture the reference's
    plot_event_cnt returns for the count image src (float32 [2,h,w]; round: rounded half-to-even first) -- include/bmc_hip.h
    "event-count images" states the contract.  Two launches for all slots (bmc_slot_render), deterministic; other slots are not
    touched.  scratch: float32 GPU tensor of at least 4 * S values (the percentiles)."""
    global RENDER_LAUNCHES
    _check(table.render > 0, "the slot table has no render tables (SlotTable(render=K))")
    _check(all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) and v >= 1 for v in (h, w))
           and h * w <= MAX_RENDER_PIXELS, "images of 1 .. 2^24 pixels can be rendered (got %r x %r)" % (h, w))
    _check(torch.is_tensor(scratch) and scratch.is_cuda and scratch.dtype == torch.float32 and scratch.is_contiguous()
           and scratch.numel() >= 4 * table.S, "scratch must be a contiguous fp32 GPU tensor of at least 4 * S values")
    lib.call(lib._slot_render, "bmc_slot_render", table.ptr(), table.render_ptr(k), table.S, int(h), int(w), int(bool(round)),
             render_parts(h, w), scratch.data_ptr(), _stream())
    RENDER_LAUNCHES += 1


def emit_parts(sH, sW):
    """Workgroups per slot of bmc_slot_emit for a [2,sH,sW] prediction (chunks of about 4 096 elements -- four tiles of a
    workgroup --, at most 1 024: 338 at 720x960, more than the chip has CUs, so one slot alone fills it)."""
    return max(1, min(MAX_EMIT_PARTS, -(-2 * sH * sW // 4096)))


def _check_emit_args(table, pred, max_count, nparts, parts, words=1):
    """The prediction and the part totals (`words` per slot and part) of emit() / emit_timed() (max_count and nparts are in
    range) -> (S, sH, sW)."""
    _check(torch.is_tensor(pred) and pred.dim() == 4 and pred.shape[1] == 2 and pred.is_cuda and pred.is_contiguous()
           and pred.dtype == torch.float32 and pred.shape[0] == table.S, "pred must be a contiguous fp32 GPU tensor [S,2,sH,sW]")
    S, _, sH, sW = pred.shape
    _check(max(sH, sW) <= MAX_COUNT_LIMIT, "predictions larger than %d pixels a side cannot be emitted (int16 coordinates)"
           % MAX_COUNT_LIMIT)
    _check(torch.is_tensor(parts) and parts.is_cuda and parts.dtype == torch.int32 and parts.is_contiguous()
           and parts.numel() >= words * S * nparts,
           "parts must be a contiguous int32 GPU tensor of at least %sS * nparts words" % ("%d * " % words if words > 1 else ""))
    _check((-(-2 * sH * sW // nparts) + 3) // 4 * 4 * max_count < 2 ** 32,
           "a part's event total would overflow 32 bits: use more parts")
    return S, sH, sW


def emit(table, pred, max_count, nparts, parts):
    """Every active slot with an emit entry: the events of pred[s] ([2,sH,sW]; q = min(rint(v), max_count) for v > 0, else 0;
    q events (x, sH-1-row, +1 / -1 by channel) per element in flat order) are appended to the entry's columns at *index_in,
    *index_out <- *index_in + their number (bmc_slot_emit: a count and a write launch for all slots, deterministic).
    parts: int32 scratch of at least S * nparts words."""
    global EMIT_LAUNCHES
    _check(table.emit, "the slot table has no emit entries (SlotTable(emit=True))")
    _check(not table.timed, "the slot table has timed emit entries: use emit_timed()")
    _check(isinstance(max_count, int) and 1 <= max_count <= MAX_COUNT_LIMIT, "1 <= max_count <= %d (got %r)"
           % (MAX_COUNT_LIMIT, max_count))
    _check(isinstance(nparts, int) and 1 <= nparts <= MAX_EMIT_PARTS, "1 <= nparts <= %d (emit)" % MAX_EMIT_PARTS)
    S, sH, sW = _check_emit_args(table, pred, max_count, nparts, parts)
    lib.call(lib._slot_emit, "bmc_slot_emit", table.ptr(), table.emit_ptr(), S, pred.data_ptr(), sH, sW, max_count, nparts,
             parts.data_ptr(), _stream())
    EMIT_LAUNCHES += 1


def voxel_parts(sH, sW):
    """Workgroups per slot of both bmc_slot_voxel launches for a [2,sH,sW] prediction (chunks of about 4 096 elements in the
    reduce launch and 2 048 pixels in the voxel launch, at most 1 024 parts: 338 at 720x960)."""
    return max(1, min(MAX_EMIT_PARTS, -(-2 * sH * sW // 4096)))


def voxel(table, pred, max_count, bins, nparts, parts):
    """Every active slot whose voxel entry has a dst: dst (float32 [bins,sH,sW]) <- the temporal-bilinear voxel grid the
    reference's events_to_voxel_torch gives for the timed event stream of pred[s] ([2,sH,sW]; q = min(rint(v), max_count) for
    v > 0, else 0), computed per pixel from its two counts -- include/bmc_hip.h "voxel grids" states the contract; the grid's
    rows are the sensor's y, flipped against the prediction's.  Two launches for all slots (bmc_slot_voxel), no atomics,
    deterministic; other slots are not touched.  parts: int32 scratch of at least 2 * S * nparts words."""
    global VOXEL_LAUNCHES
    _check(table.voxel, "the slot table has no voxel entries (SlotTable(voxel=True))")
    _check(not isinstance(max_count, bool) and isinstance(max_count, int) and 1 <= max_count <= MAX_COUNT_TIMED,
           "voxel grids need 1 <= max_count <= %d (got %r)" % (MAX_COUNT_TIMED, max_count))
    _check(not isinstance(bins, bool) and isinstance(bins, (int, np.integer)) and 1 <= bins <= MAX_VOXEL_BINS,
           "1 <= bins <= %d (got %r)" % (MAX_VOXEL_BINS, bins))
    _check(not isinstance(nparts, bool) and isinstance(nparts, int) and 1 <= nparts <= MAX_EMIT_PARTS,
           "1 <= nparts <= %d (voxel)" % MAX_EMIT_PARTS)
    _check(torch.is_tensor(parts) and parts.numel() >= 2 * table.S * nparts,
           "parts must be a contiguous int32 GPU tensor of at least 2 * S * nparts words")
    S, sH, sW = _check_emit_args(table, pred, max_count, nparts, parts)
    lib.call(lib._slot_voxel, "bmc_slot_voxel", table.ptr(), table.voxel_ptr(), S, pred.data_ptr(), sH, sW, max_count, int(bins),
             nparts, parts.data_ptr(), _stream())
    VOXEL_LAUNCHES += 1


def quality_tiles(gh, gw):
    """Workgroups per (slot, image, channel) of bmc_slot_quality's ssim launch for a gh x gw ground truth: the tiles of
    QUALITY_TILE_H x QUALITY_TILE_W window positions that cover its (gh - 6) x (gw - 6) positions."""
    _check(min(gh, gw) >= QUALITY_WIN, "PSNR / SSIM need images of at least %d x %d (got %d x %d)" % (QUALITY_WIN, QUALITY_WIN, gh, gw))
    return -(-(gh - QUALITY_WIN + 1) // QUALITY_TILE_H) * -(-(gw - QUALITY_WIN + 1) // QUALITY_TILE_W)


def check_data_range(who, data_range):
    """data_range ("gt", or a finite positive number) -> the constant bmc_slot_quality takes (0.0 for "gt"); ValueError otherwise."""
    if isinstance(data_range, str) and data_range == "gt":
        return 0.0
    if isinstance(data_range, (bool, str)) or not isinstance(data_range, (int, float, np.integer, np.floating)) \
            or not np.isfinite(data_range) or not data_range > 0:
        raise ValueError(who + "data_range must be 'gt' or a finite positive number (got %r)" % (data_range,))
    return float(data_range)


def quality(table, esr, bicubic, nparts, data_range, stats, tiles):
    """Every active slot with a ground truth whose quality entry has a dst: dst (float64 [2,2,QUALITY_WORDS]) <- the raw records
    {sse, gt_max, gt_min, ssim_sum} per channel of the images esr[s] and bicubic[s] (fp32 [S,2,gh,gw], at the ground truth's
    size; bicubic None: the first image only) against the slot entry's gt -- include/bmc_hip_quality.h states the contract.
    data_range: 0.0 (from the ground truth) or the constant.  Three launches for all slots (bmc_slot_quality), no atomics,
    deterministic; other slots are not touched.  stats / tiles: float64 scratch of at least S * nparts * QUALITY_STATS_WORDS and
    S * 4 * quality_tiles(gh, gw) values."""
    global QUALITY_LAUNCHES
    _check(table.quality, "the slot table has no quality entries (SlotTable(quality=True))")
    _check(torch.is_tensor(esr) and esr.dim() == 4 and esr.shape[1] == 2 and esr.is_cuda and esr.is_contiguous()
           and esr.dtype == torch.float32 and esr.shape[0] == table.S, "esr must be a contiguous fp32 GPU tensor [S,2,gh,gw]")
    S, _, gh, gw = esr.shape
    _check(bicubic is None or (torch.is_tensor(bicubic) and bicubic.is_cuda and bicubic.is_contiguous()
                               and bicubic.dtype == torch.float32 and bicubic.shape == esr.shape),
           "bicubic must be None or a contiguous fp32 GPU tensor of esr's shape")
    _check(not isinstance(nparts, bool) and isinstance(nparts, int) and 1 <= nparts <= MAX_PARTS, "1 <= nparts <= %d" % MAX_PARTS)
    _check(2 * gh * gw < 2 ** 30, "images of fewer than 2^29 pixels")
    ntiles = quality_tiles(gh, gw)
    for name, t, need in (("stats", stats, S * nparts * QUALITY_STATS_WORDS), ("tiles", tiles, S * 4 * ntiles)):
        _check(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() >= need,
               "%s must be a contiguous float64 GPU tensor of at least %d values" % (name, need))
    lib.call(quality_lib._slot_quality, "bmc_slot_quality", table.ptr(), table.quality_ptr(), S, esr.data_ptr(),
             None if bicubic is None else bicubic.data_ptr(), gh, gw, nparts, float(data_range), stats.data_ptr(),
             tiles.data_ptr(), _stream())
    QUALITY_LAUNCHES += 1


def quality_values(raw, data_range, size):
    """Raw records [..., 2 channels, QUALITY_WORDS] = {sse, gt_max, gt_min, ssim_sum} of bmc_slot_quality for images of
    size = (gh, gw) (float64; numpy, or a tensor on any device) -> (psnr [...], ssim [...]) numpy float64, the mean of the two
    channels' values: psnr_c = 10 log10(R_c^2 / (sse / (gh gw))), ssim_c = ssim_sum / ((gh - 6)(gw - 6)), R_c = gt_max - gt_min
    for data_range "gt", else the constant.  IEEE results stand (numpy float64, errstate ignore): +inf for an exact channel,
    -inf for R_c = 0 with an error, nan for 0 / 0; ssim is nan where R_c = 0 (the kernel wrote a nan sum)."""
    rng = check_data_range("slots.quality_values: ", data_range)
    gh, gw = (int(v) for v in size)
    _check(min(gh, gw) >= QUALITY_WIN, "PSNR / SSIM need images of at least %d x %d (got %d x %d)" % (QUALITY_WIN, QUALITY_WIN, gh, gw))
    raw = np.asarray(raw.cpu() if torch.is_tensor(raw) else raw, dtype=np.float64)
    _check(raw.ndim >= 2 and raw.shape[-2:] == (2, QUALITY_WORDS), "raw records are [..., 2, %d] (got %s)" % (QUALITY_WORDS, raw.shape))
    sse, gt_max, gt_min, ssim_sum = (raw[..., k] for k in range(QUALITY_WORDS))
    R = gt_max - gt_min if rng == 0.0 else np.full_like(sse, rng)
    with np.errstate(all="ignore"):
        psnr = 10.0 * np.log10(R * R / (sse / np.float64(gh * gw)))
        ssim = ssim_sum / np.float64((gh - QUALITY_WIN + 1) * (gw - QUALITY_WIN + 1))
        return (psnr[..., 0] + psnr[..., 1]) / 2.0, (ssim[..., 0] + ssim[..., 1]) / 2.0


def emit_rank_table_np():
    """[256][256] uint16: table[n][j] (0 <= j < n) = the dense rank of the rational j / (n - 1) (0 for n = 1) among all
    fractions p/d with 1 <= d <= 254, 0 <= p <= d -- the sort key of the timed event output (include/bmc_hip.h).  Integer
    arithmetic only: floor(j * 2^40 / (n - 1)) is equal for equal rationals, and distinct ones (at least 1 / (254 * 253)
    apart) differ by more than 10^7, so the ranks of the distinct floors are the ranks of the rationals."""
    n, j = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    valid = (j < n) & (n >= 2)
    key = np.where(valid, (j << 40) // np.maximum(n - 1, 1), 0)       # n = 1, j = 0: the rational 0
    ranks = np.unique(key[valid], return_inverse=True)[1]
    table = np.zeros((256, 256), np.int64)
    table[valid] = ranks
    assert table.max() < 1 << 16
    return table.astype(np.uint16)


def emit_rank_table(device):
    """The rank table on `device` (uploaded once per device; int16 storage of the uint16 bits)."""
    device = torch.device(device)
    if device not in _RANK_TABLES:
        _RANK_TABLES[device] = torch.from_numpy(emit_rank_table_np().view(np.int16)).to(device)
    return _RANK_TABLES[device]


def _check_window_capacity(window_capacity):
    _check(not isinstance(window_capacity, bool) and isinstance(window_capacity, (int, np.integer))
           and 1 <= window_capacity <= MAX_WINDOW_CAPACITY,
           "window_capacity must be an integer, 1 <= window_capacity <= %d (got %r)" % (MAX_WINDOW_CAPACITY, window_capacity))


def emit_timed_scratch_bytes(S, nparts, window_capacity):
    """Bytes of sort scratch of emit_timed for S slots: 8 per event of window_capacity per slot, and the digit histograms."""
    _check(1 <= S <= MAX_SLOTS, "1 <= S <= %d" % MAX_SLOTS)
    _check(isinstance(nparts, int) and 1 <= nparts <= MAX_EMIT_PARTS, "1 <= nparts <= %d (emit)" % MAX_EMIT_PARTS)
    _check_window_capacity(window_capacity)
    return int(lib._slot_emit_timed_ws(S, nparts, int(window_capacity)))


def emit_timed(table, pred, max_count, nparts, parts, scratch, window_capacity):
    """emit() with times, every window in time order (bmc_slot_emit_timed; include/bmc_hip.h states the contract): event j of
    an element with n events has t = float32(T0 + (T1 - T0) * j / (n - 1)); the window is sorted by the exact rational
    j / (n - 1), ties in flat emission order, and appended to the entry's xs / ys / ps / ts columns at *index_in;
    *index_out <- *index_in + the window's event count.  A window of more than window_capacity events stores nothing.
    parts: int32 scratch of at least S * nparts words; scratch: uint8, emit_timed_scratch_bytes(S, nparts, window_capacity)."""
    _emit_timed(False, table, pred, max_count, nparts, parts, scratch, window_capacity)


def emit_clocked(table, pred, max_count, nparts, parts, scratch, window_capacity):
    """emit_timed() on a table with clock entries (bmc_slot_emit_clocked; include/bmc_hip.h states the contract): a slot whose
    clock entry has a `ts` column stores float64 times t = t_first + tau * (t_last - t_first) there, tau from the reduced
    fraction of j / (n - 1); a slot without one gets emit_timed()'s float32 column.  Same events, order, capacity rules,
    arguments and launches (counted in EMIT_TIMED_LAUNCHES)."""
    _check(table.clock, "the slot table has no clock entries (SlotTable(emit=True, timed=True, clock=True))")
    _emit_timed(True, table, pred, max_count, nparts, parts, scratch, window_capacity)


def emit_trimmed(table, pred, max_count, nparts, parts, scratch, window_capacity):
    """emit_clocked() on a table with trim entries (bmc_slot_emit_trimmed; include/bmc_hip_stream.h states the contract): a
    clocked slot emits exactly the events of emit_clocked() whose float64 time is < its trim entry's t_cut -- a prefix of the
    sorted window, with the same bytes -- found BEFORE the sort; *index_out <- *index_in + the kept count, both capacity rules
    apply to the kept events, and the entry's `dropped` address (0: none) receives the number of events cut off.  A slot
    without a `ts` column in its clock entry is not trimmed.  The arguments and launches of emit_clocked() (counted in
    EMIT_TIMED_LAUNCHES), but parts: at least stream_lib.TRIM_PARTS * S * nparts words."""
    _check(table.clock and getattr(table, "trim", False),
           "the slot table has no trim entries (SlotTable(emit=True, timed=True, clock=True, trim=True))")
    _emit_timed("trimmed", table, pred, max_count, nparts, parts, scratch, window_capacity)


def _emit_timed(clocked, table, pred, max_count, nparts, parts, scratch, window_capacity):
    global EMIT_TIMED_LAUNCHES
    _check(table.emit and table.timed,
           "the slot table has no timed emit entries (SlotTable(emit=True, timed=True))")
    _check(not isinstance(max_count, bool) and isinstance(max_count, int) and 1 <= max_count <= MAX_COUNT_TIMED,
           "timed emission needs 1 <= max_count <= %d (got %r)" % (MAX_COUNT_TIMED, max_count))
    _check(isinstance(nparts, int) and 1 <= nparts <= MAX_EMIT_PARTS, "1 <= nparts <= %d (emit)" % MAX_EMIT_PARTS)
    _check_window_capacity(window_capacity)
    S, sH, sW = _check_emit_args(table, pred, max_count, nparts, parts, stream_lib.TRIM_PARTS if clocked == "trimmed" else 1)
    need = emit_timed_scratch_bytes(S, nparts, window_capacity)
    _check(torch.is_tensor(scratch) and scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous()
           and scratch.numel() >= need and scratch.data_ptr() % 8 == 0,
           "scratch must be a contiguous 8-byte aligned uint8 GPU tensor of at least %d bytes" % need)
    tail = (S, pred.data_ptr(), sH, sW, max_count, nparts, parts.data_ptr(), emit_rank_table(pred.device).data_ptr(),
            scratch.data_ptr(), int(window_capacity), _stream())
    if clocked == "trimmed":
        lib.call(stream_lib._slot_emit_trimmed, "bmc_slot_emit_trimmed", table.ptr(), table.emit_ptr(), table.clock_ptr(),
                 table.trim_ptr(), *tail)
    elif clocked:
        lib.call(lib._slot_emit_clocked, "bmc_slot_emit_clocked", table.ptr(), table.emit_ptr(), table.clock_ptr(), *tail)
    else:
        lib.call(lib._slot_emit_timed, "bmc_slot_emit_timed", table.ptr(), table.emit_ptr(), *tail)
    EMIT_TIMED_LAUNCHES += 1
