"""Streaming single-GPU inference with the reference's semantics (infer_BMCNet.py:20-103):
the recurrent state (h, h_p, h_n, previous HR prediction) is created once and carried across calls, every call
runs one window under no_grad, and the per-window latency is measured with events on the launch stream exactly
where the reference puts its `starter/ender` pair (infer_BMCNet.py:54,66-68).

MultiStreamSR runs many recordings through one model at once (slots of one batched window); evaluate_recordings is the
reference's evaluation mode 1 on top of it.  A recording is handed over as count images (open) or as the dataset's raw event
columns with the index tables of its blocks (open_events, EventRecording), encoded window by window on the GPU.  With
emit_events the result leaves the same way: the super-resolved event stream of every window, in the dataset's column format."""
import collections
import statistics

import numpy as np
import torch

EventRecording = collections.namedtuple("EventRecording", "lr gt lr_index gt_index lr_size gt_size", defaults=(None,) * 5)
EventRecording.__doc__ = """An event-backed recording for MultiStreamSR.open_events / evaluate_recordings: lr, gt = (xs, ys, ps)
raw dataset columns on the GPU (int16, int16, float64); lr_index, gt_index [L,2] = the event range [first, end) of every
item's LR / ground-truth frame (bmc_hip.encodings.event_window_indices); lr_size = (H, W), gt_size = (gh, gw).  A recording
without ground truth: gt = gt_index = gt_size = None."""


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


class MultiStreamSR:
    """Many recordings through one model at once: S slots of one batched forward pass, each carrying its own recording's
    recurrent state; a recording that ends frees its slot for the next queued one (infer_BMCNet.py mode 1, :248-295, runs
    them one after another at batch 1).  Per window: bmc_slot_stage (inputs + state, exact zeros where a recording starts),
    the model under no_grad with init=False (a zero state and a zero previous prediction give what init=True gives), then
    bmc_slot_commit (state back to the pool) and bmc_slot_metrics (esr_mse / bicubic_mse sums per slot, read only when
    results() asks) -- one launch each for all slots (bmc_hip/slots.py).

    open(frames [L,2,H,W], gts [L,2,gh,gw]) queues a recording (fp32, on the GPU; windows as oracle.infer_windows: `seqn`
    frames each, the ground truth of window i is frame i+1); step() runs one window for every active slot; run() steps to the
    end; results(handle) gives per-window esr_mse, bicubic_mse, time (ms, events on the launch stream around the whole
    window, shared by the slots of that window) and, with keep_predictions, the predictions [n_windows,2,sH,sW].

    open_events(lr, gt, lr_index, gt_index, lr_size, gt_size) queues an EVENT-BACKED recording: the raw dataset columns stay
    on the GPU (12 bytes per event instead of 8 bytes per pixel of every frame) and the frames of a window are encoded on the
    fly by bmc_slot_encode -- one more launch per window for all slots, into per-slot scratch that the slot's table entry
    points at; the other kernels do not know the difference, and the results are bit-identical to open() on the frames the
    raw-column encoder (ops.encode_raw_events, no flips) gives for the same ranges.  The encode launch is issued only once an
    event-backed recording has been opened; both kinds may share a session.

    graph=True: from the third window on a window is ONE graph replay ([encode,] stage, forward, commit, metrics captured; the
    slot table is refreshed by one small copy before it); the first open_events after a capture invalidates the graph.  Parameter updates invalidate the graph as in StreamingSR.
    state_dtype=torch.bfloat16: the feature states rest in bf16 between windows, as StreamingSR(state_dtype=bf16).

    emit_events=True: every window's prediction is also turned into an EVENT LIST on the GPU (bmc_slot_emit: two more launches
    per window for all slots, inside the captured graph too) and appended to the recording's own output columns: per element v
    of the prediction [2,sH,sW] in flat order, q = min(rint(v), max_count) for v > 0 (else 0; round-half-to-even -- the rounded
    count image the reference renders, infer_BMCNet.py:94) events xs = x, ys = sH-1-row, ps = +1 (channel 0) / -1 (channel 1),
    so that encoding a window's events at (sH, sW) gives q back exactly.  results() then carries sr_events = (xs int16, ys int16,
    ps int8) and sr_index [done+1] (window i owns events [sr_index[i], sr_index[i+1])); without event_times there are no
    timestamps and a window's events are in pixel order.  The columns hold `event_capacity` events (open / open_events; default 2 x scale^2 x the recording's LR
    events); the index keeps counting past it, and results() then raises with the capacity that is needed.  About 5 bytes per
    event instead of 8 x sH x sW bytes per window of keep_predictions; both may be on.

    event_times="linear" (with emit_events; needs max_count <= 255): the list becomes a STREAM.  Every event also carries a
    float32 time inside its window and a window's events are stored in time order (bmc_slot_emit_timed: six launches per
    window instead of the two, inside the captured graph too) -- the reference's linear redistribution of a count image
    (dataloader/encodings.py:367-414, mode='linear', one time bin): event j of a pixel's n events has t = 0.01 + 0.99 * j /
    (n - 1) (0.01 for n = 1; float64, rounded once), the window is sorted by the exact j / (n - 1), ties in the pixel order
    above.  results() then also carries sr_ts (float32, on the GPU), parallel to sr_events.  Times are window-normalised: a
    count image has no absolute clock.  The sort works in per-slot scratch of `window_event_capacity` events (open /
    open_events; default 2 x scale^2 x the LR events of the recording's busiest frame, at most 2 x sH x sW x max_count); a
    window that emits more stores nothing, the index keeps the true count and results() raises with the capacity needed.

    Recordings WITHOUT ground truth (open(frames), open_events(lr, None, lr_index, None, lr_size)): what a deployed sensor
    delivers.  Their results() carry no esr_mse / bicubic_mse; they only have to match the session's (H, W) and may share it
    with recordings that have a ground truth.  bmc_slot_metrics is launched only once a recording with ground truth has been
    opened (the first such open after a capture invalidates the graph, as the first open_events does).

    Events on the SENSOR'S CLOCK (event_times="linear"; open(..., spans=) / open_events(..., lr_ts= or spans=)): spans [L,2]
    float64 = (t_first, t_last) of every item on the recording's own time base (open_events derives them from the timestamp
    column lr_ts: bmc_hip.encodings.event_block_spans).  Window i predicts item i+1 (infer_BMCNet.py:52) and uses its span:
    sr_ts is then FLOAT64, t = t_first + tau * (t_last - t_first) with tau the window time above computed from the reduced
    fraction of j / (n - 1) (bmc_slot_emit_clocked; include/bmc_hip.h states the contract) -- the inverse of
    event_formatting's normalisation (dataloader/base_dataset.py:30) without its 1e-6.  Each window is in time order; with
    sliding_window < window the spans of consecutive windows overlap, so the concatenation of a recording's windows is
    globally sorted only for non-overlapping spans.  Clocked and unclocked recordings may share a session.

    hot_filter=dict(max_px=, min_obvs=, max_rate=): the reference's hot-pixel filter (dataset.hot_filter; create_hot_mask,
    dataloader/h5dataset.py:528-548; get_hot_event_mask, dataloader/encodings.py:349-364) on the GPU, for recordings opened with
    open_events: every LR item is observed once, in item order (a per-slot count of the items in which a pixel fired), its mask
    follows the reference's rule bit for bit, and the item's count image has both channels zeroed where the mask says so --
    include/bmc_hip.h states the contract.  bmc_slot_hot_update (one more launch per window for all slots, inside the captured
    graph too) runs before the encode launch, which becomes bmc_slot_encode_filtered.  Recordings opened with open() in the same
    session stay UNFILTERED, and so does every ground truth.  results() then carries hot_pixels (per window, the number of
    pixels masked for the item that window newly observed) and hot_mask ([H,W] uint8 in sensor coordinates, 1 = kept, of the
    last item observed).  The option needs nothing else switched on.

    render=(kinds...) from ("lr", "bicubic", "esr", "gt"): the four EVENT-COUNT IMAGES the reference's inference writes per
    window (infer_BMCNet.py:90-97: lr_event_img, hr_bicubic_event_img, hr_esr_event_img, hr_gt_event_img), rendered on the GPU as
    the uint8 [h,w,3] arrays its plot_event_cnt returns, byte for byte (bmc_slot_render: two launches per kind for all slots,
    inside the captured graph too; include/bmc_hip.h "event-count images" states the contract).  lr: frame 1 of the window as
    the model sees it (H x W; after the hot-pixel filter where one applies); esr: the prediction, resized to the ground truth's
    size where that differs (bmc_bicubic_resize_fwd, as the metric does) and rounded half-to-even; bicubic: frame 1 resized to
    the ground truth's size; gt: the window's ground truth.  A recording without ground truth gets lr and esr (at the
    prediction's size) only.  results() then carries images = {kind: uint8 [done,h,w,3]} on the GPU: 3 bytes per pixel and
    window instead of the 8 of keep_predictions.  None (the default): no image, no launch.

    voxel_bins=B (1 <= B <= 32; needs max_count <= 255): every window's prediction also leaves as the temporal-bilinear VOXEL
    GRID of its super-resolved events, the input form of reconstruction, flow and recognition networks: what the reference's
    events_to_voxel_torch (dataloader/encodings.py:100-148) returns for the window's timed event stream (the stream of
    event_times="linear"), bit for bit, computed per output pixel from the prediction's two counts and one small reduction
    (bmc_slot_voxel: two more launches per window for all slots, inside the captured graph too; no sort, no atomics, no event
    storage; include/bmc_hip.h "voxel grids" states the contract).  Independent of emit_events, event_times and render, for
    frame-backed and event-backed recordings, with or without ground truth.  results() then carries voxels = float32
    [done,B,sH,sW] on the GPU, at the prediction's own size; its rows are the sensor's y, vertically flipped against the
    prediction's rows as the emitted ys are.  The grid is window-normalised, so a sensor clock does not change it.  Resident:
    4 x B x sH x sW bytes per window -- 13.8 MB per window at 720x960 with 5 bins.  None (the default): no grid, no launch, no
    table section."""

    MAX_VOXEL_BINS = 32          # BMC_SLOT_VOXEL_MAX_BINS
    RENDER_KINDS = ("lr", "bicubic", "esr", "gt")
    MAX_COUNT_LIMIT = 32767      # emitted counts and coordinates are int16
    MAX_COUNT_TIMED = 255        # event_times: the sort key is a 16-bit rank of j / (n - 1), n <= 255
    MAX_WINDOW_CAPACITY = 1 << 28

    def __init__(self, model, slots, n_c=128, scale=4, plain=False, graph=False, state_dtype=None, keep_predictions=False,
                 seqn=3, emit_events=False, max_count=255, event_times=None, hot_filter=None, render=None, voxel_bins=None):
        from bmc_hip.slots import check_hot_filter
        self.hot_filter = check_hot_filter("MultiStreamSR: ", hot_filter)
        self.render = self.check_render("MultiStreamSR: ", render)
        if state_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError("MultiStreamSR: state_dtype must be None / torch.float32 / torch.bfloat16 (got %r)" % (state_dtype,))
        if seqn < 2:
            raise ValueError("MultiStreamSR: seqn >= 2 (the model reads frames 0 and 1 of a window)")
        if isinstance(max_count, bool) or not isinstance(max_count, int) or not 1 <= max_count <= self.MAX_COUNT_LIMIT:
            raise ValueError("MultiStreamSR: max_count must be an integer, 1 <= max_count <= %d (got %r)"
                             % (self.MAX_COUNT_LIMIT, max_count))
        if event_times not in (None, "linear"):
            raise ValueError("MultiStreamSR: event_times must be None or 'linear' (got %r)" % (event_times,))
        if event_times is not None and not emit_events:
            raise ValueError("MultiStreamSR: event_times needs emit_events=True")
        if event_times is not None and max_count > self.MAX_COUNT_TIMED:
            raise ValueError("MultiStreamSR: event_times needs max_count <= %d (got %d)" % (self.MAX_COUNT_TIMED, max_count))
        if voxel_bins is not None:
            if isinstance(voxel_bins, bool) or not isinstance(voxel_bins, (int, np.integer)) or not 1 <= voxel_bins <= self.MAX_VOXEL_BINS:
                raise ValueError("MultiStreamSR: voxel_bins must be None or an integer, 1 <= voxel_bins <= %d (got %r)"
                                 % (self.MAX_VOXEL_BINS, voxel_bins))
            if max_count > self.MAX_COUNT_TIMED:
                raise ValueError("MultiStreamSR: voxel_bins needs max_count <= %d (the timed stream's limit; got %d)"
                                 % (self.MAX_COUNT_TIMED, max_count))
            voxel_bins = int(voxel_bins)
        self.voxel_bins = voxel_bins
        self.event_times = event_times
        self._wcap = 0             # events per window the sort scratch holds (the largest window_event_capacity so far)
        self.model = model.eval()
        self.S, self.n_c, self.scale, self.plain, self.seqn = int(slots), n_c, scale, plain, int(seqn)
        self.use_graph = graph
        self.state_dtype = None if state_dtype is torch.float32 else state_dtype
        self.keep_predictions = keep_predictions
        self.emit_events, self.max_count = bool(emit_events), max_count
        self.sched = SlotScheduler(self.S)
        self.replays = 0
        self._recs = {}
        self._size = None          # (H, W) of the first recording, (H, W, gh, gw) once one with ground truth has been opened
        self._bufs = None
        self._steps = []           # (start, end) events per window
        self._calls = 0
        self._graph = self._stamp = None
        self._has_events = False
        self._has_clock = False

    @classmethod
    def check_render(cls, who, render):
        """render (None, or a tuple / list of distinct kinds from RENDER_KINDS) -> the kinds in RENDER_KINDS' order (() for None);
        ValueError naming what is wrong."""
        if render is None:
            return ()
        if isinstance(render, str) or not isinstance(render, (tuple, list)) or not render:
            raise ValueError(who + "render must be None or a non-empty tuple of kinds from %s (got %r)" % (cls.RENDER_KINDS, render))
        for k in render:
            if not isinstance(k, str) or k not in cls.RENDER_KINDS:
                raise ValueError(who + "render has an unknown kind %r (the kinds are %s)" % (k, ", ".join(cls.RENDER_KINDS)))
        if len(set(render)) != len(render):
            raise ValueError(who + "render names a kind twice (got %r)" % (render,))
        return tuple(k for k in cls.RENDER_KINDS if k in render)

    # the render tables of the slot table: "esr" draws from the prediction, "esr_gt" from the prediction resized to the ground truth
    RENDER_TABLES = ("lr", "esr", "esr_gt", "bicubic", "gt")

    def _render_size(self, kind, has_gt):
        """(h, w) of a recording's image of `kind`."""
        H, W = self._size[:2]
        if kind == "lr":
            return H, W
        return tuple(self._size[2:]) if has_gt else (self.scale * H, self.scale * W)

    # ---------------------------------------------------------------- recordings
    def _check_capacities(self, who, event_capacity, capacity):
        """The two capacities a caller of open / open_events may give (None: the default)."""
        if event_capacity is not None:
            if not self.emit_events:
                raise ValueError("MultiStreamSR.%s: event_capacity needs a session with emit_events=True" % who)
            if isinstance(event_capacity, bool) or not isinstance(event_capacity, (int, np.integer)) or event_capacity < 1:
                raise ValueError("MultiStreamSR.%s: event_capacity must be a positive integer (got %r)" % (who, event_capacity))
        if capacity is not None:
            if self.event_times is None:
                raise ValueError("MultiStreamSR.%s: window_event_capacity needs a session with event_times='linear'" % who)
            if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not 1 <= capacity <= self.MAX_WINDOW_CAPACITY:
                raise ValueError("MultiStreamSR.%s: window_event_capacity must be a positive integer, at most %d (got %r)"
                                 % (who, self.MAX_WINDOW_CAPACITY, capacity))

    def _emit_room(self, who, H, W, event_capacity, window_event_capacity, total, busiest):
        """What an emitting session needs of a recording of H x W frames: coordinates in int16, and the two capacities, by
        default 2 x scale^2 x the recording's LR events / 2 x scale^2 x the LR events of its busiest item (at most what a window
        can emit).  total / busiest give those counts and are called only where a default is needed."""
        if self.emit_events and max(self.scale * H, self.scale * W) > self.MAX_COUNT_LIMIT:
            raise ValueError("MultiStreamSR.%s: predictions of %d x %d cannot be emitted (int16 coordinates)"
                             % (who, self.scale * H, self.scale * W))
        if self.emit_events and event_capacity is None:
            event_capacity = 2 * self.scale ** 2 * int(total())
        if self.event_times is not None and window_event_capacity is None:
            most = 2 * self.scale ** 2 * H * W * self.max_count
            window_event_capacity = max(1, min(2 * self.scale ** 2 * int(busiest()), most, self.MAX_WINDOW_CAPACITY))
        return event_capacity, window_event_capacity

    def _check_spans(self, who, spans, L):
        """spans (or None) -> a validated [L,2] float64 table on the host (or None)."""
        if spans is None:
            return None
        if self.event_times is None:
            raise ValueError("MultiStreamSR.%s: spans / lr_ts need a session with event_times='linear'" % who)
        from bmc_hip.encodings import check_spans
        return check_spans("MultiStreamSR.%s: " % who, spans, L)

    def open(self, frames, gts=None, gt_size=None, event_capacity=None, window_event_capacity=None, spans=None):
        """Queue one recording -> handle.  frames [L,2,H,W], gts [L,2,gh,gw] (fp32, on the GPU); gt_size (the reference's
        gt_sensor_resolution, the bicubic baseline's size) must be the ground truth's size.  gts=None: a recording without
        ground truth (no metrics).  event_capacity (emit_events): events the output columns hold; default 2 x scale^2 x the
        sum of `frames` (one device reduction here).  window_event_capacity (event_times): events of ONE window the sort
        scratch holds; default 2 x scale^2 x the largest sum of one frame.  spans (event_times) [L,2] float64 on the host:
        (t_first, t_last) of every frame on the sensor's clock -> sr_ts is float64 on that clock."""
        self._check_capacities("open", event_capacity, window_event_capacity)
        given = (frames,) if gts is None else (frames, gts)
        if frames.dim() != 4 or frames.shape[1] != 2 or any(g.dim() != 4 or tuple(g.shape[:2]) != (frames.shape[0], 2)
                                                            for g in given[1:]):
            raise ValueError("MultiStreamSR.open: frames [L,2,H,W]%s (got %s)"
                             % (" and gts [L,2,gh,gw]" * (gts is not None), ", ".join(str(tuple(g.shape)) for g in given)))
        if gts is None and gt_size is not None:
            raise ValueError("MultiStreamSR.open: gt_size without a ground truth")
        spans = self._check_spans("open", spans, frames.shape[0])
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
        event_capacity, window_event_capacity = self._emit_room(
            "open", H, W, event_capacity, window_event_capacity, lambda: frames.sum(dtype=torch.float64).item(),
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
                from bmc_hip import slots
                self._nparts = slots.emit_parts(self.scale * H, self.scale * W)
                self._vparts = slots.voxel_parts(self.scale * H, self.scale * W)
            self._size = size
            if len(size) == 4:                             # a running session without ground truth: the metrics launch joins
                self._grow(self._gt_scratch, self._render_buffers)

    def _grow(self, *rebuild):
        """The session gains a part (a first event-backed, clocked or ground-truth recording, a larger window capacity).  One
        that has run already rebuilds the buffers concerned -- rebuild: methods taking (buffers, device) -- and drops its
        captured graph, which holds the old addresses and launches."""
        if self._bufs is not None:
            for make in rebuild:
                make(self._bufs, self._bufs["x"].device)
            self.invalidate()

    def _add(self, rec, L, device, event_capacity=None, window_event_capacity=None, spans=None):
        """Queue a recording of L items (frames or event blocks) -> handle."""
        from bmc_hip import slots
        H, W = self._size[:2]
        nwin = L - self.seqn + 1
        if "gts" in rec or "gt" in rec:                    # the result sums of a recording with ground truth
            rec["sse"] = torch.zeros(nwin, slots.metric_parts(*self._size[2:]), 2, dtype=torch.float64, device=device)
        rec.update(n=nwin, steps=[], device=device,
                   keep=torch.empty(nwin, 2, self.scale * H, self.scale * W, device=device) if self.keep_predictions else None)
        if self.render:                                    # the recording's pictures: without ground truth, lr and esr only
            has_gt = "sse" in rec
            if max(h * w for h, w in (self._render_size(k, has_gt) for k in self.render)) > slots.MAX_RENDER_PIXELS:
                raise ValueError("MultiStreamSR: images of more than 2^24 pixels cannot be rendered (sizes %s)" % (self._size,))
            rec["images"] = {k: torch.empty((nwin,) + self._render_size(k, has_gt) + (3,), dtype=torch.uint8, device=device)
                             for k in self.render if has_gt or k in ("lr", "esr")}
        if self.voxel_bins is not None:                    # the recording's voxel grids, at the prediction's size
            if max(self.scale * H, self.scale * W) > self.MAX_COUNT_LIMIT:
                raise ValueError("MultiStreamSR: predictions of %d x %d are too large for voxel grids (at most %d a side)"
                                 % (self.scale * H, self.scale * W, self.MAX_COUNT_LIMIT))
            rec["voxels"] = torch.empty(nwin, self.voxel_bins, self.scale * H, self.scale * W, device=device)
        if self.emit_events:                               # the recording's output stream: three columns and the index table
            cap = max(int(event_capacity), 1)
            rec.update(ev_capacity=cap, ev_xs=torch.empty(cap, dtype=torch.int16, device=device),
                       ev_ys=torch.empty(cap, dtype=torch.int16, device=device),
                       ev_ps=torch.empty(cap, dtype=torch.int8, device=device),
                       ev_index=torch.zeros(nwin + 1, dtype=torch.int64, device=device))
        if self.event_times is not None:                   # ... a time column, and room for its largest window in the sort
            rec.update(ev_ts=torch.empty(cap, dtype=torch.float32 if spans is None else torch.float64, device=device),
                       win_capacity=int(window_event_capacity))
            if spans is not None:                          # a clocked recording: float64 times on its own clock
                rec["spans"] = spans
                if not self._has_clock:
                    self._has_clock = True
                    self._grow(self._new_table)            # the table grows a clock part
            if rec["win_capacity"] > self._wcap:
                self._wcap = rec["win_capacity"]
                self._grow(self._sort_buffers)             # the sort scratch grows
        h = self.sched.add(nwin)
        self._recs[h] = rec
        return h

    MAX_ITEMS_FILTERED = 1 << 23 # hot_filter: below it distinct counts give distinct float32 rates (include/bmc_hip.h)
    MAX_SEQN_EVENTS = 8          # bmc_slot_events_t holds the ranges of at most 8 LR frames (BMC_SLOT_MAX_SEQN)
    MAX_WIDTH_EVENTS = 7680      # bmc_slot_encode: one row of both channels must fit a workgroup's LDS band

    def open_events(self, lr, gt=None, lr_index=None, gt_index=None, lr_size=None, gt_size=None, event_capacity=None,
                    window_event_capacity=None, lr_ts=None, spans=None):
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
        (not both)."""
        who = "MultiStreamSR.open_events: "
        self._check_capacities("open_events", event_capacity, window_event_capacity)
        if lr_index is None or lr_size is None:
            raise ValueError(who + "lr_index and lr_size are required")
        has_gt = gt is not None
        if (gt_index is not None) != has_gt or (gt_size is not None) != has_gt:
            raise ValueError(who + "gt, gt_index and gt_size are all given or all None")
        if lr_ts is not None and spans is not None:
            raise ValueError(who + "give lr_ts or spans, not both")
        if (lr_ts is not None or spans is not None) and self.event_times is None:
            raise ValueError(who + "spans / lr_ts need a session with event_times='linear'")
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
        if self.hot_filter is not None:
            if L >= self.MAX_ITEMS_FILTERED:
                raise ValueError(who + "a filtered session takes recordings of fewer than 2^23 items (got %d)" % L)
            if int((lr_index[:, 1] - lr_index[:, 0]).max()) >= 2 ** 31:
                raise ValueError(who + "a filtered session takes LR items of fewer than 2^31 events")
        if lr_ts is not None:
            if not ((torch.is_tensor(lr_ts) and lr_ts.dtype == torch.float64 and lr_ts.dim() == 1) or
                    (isinstance(lr_ts, np.ndarray) and lr_ts.dtype == np.float64 and lr_ts.ndim == 1)) \
                    or len(lr_ts) != lr[0].numel() or len(lr_ts) < 1:
                raise ValueError(who + "lr_ts must be a 1-D float64 column parallel to lr[0]")
            from bmc_hip.encodings import event_block_spans
            spans = event_block_spans(lr_ts, lr_index)
        spans = self._check_spans("open_events", spans, L)
        try:
            (H, W), (gh, gw) = (int(v) for v in lr_size), ((int(v) for v in gt_size) if has_gt else (None, None))
        except (TypeError, ValueError):
            raise ValueError(who + "lr_size = (H, W) and gt_size = (gh, gw)") from None
        if min(H, W, gh or 1, gw or 1) < 1 or max(W, gw or 1) > self.MAX_WIDTH_EVENTS:
            raise ValueError(who + "sizes must be positive and at most %d wide (got %s, %s)"
                             % (self.MAX_WIDTH_EVENTS, (H, W), (gh, gw)))
        lengths = lr_index[:, 1] - lr_index[:, 0]
        event_capacity, window_event_capacity = self._emit_room("open_events", H, W, event_capacity, window_event_capacity,
                                                                lengths.sum, lengths.max)
        cols = tuple(lr) + (tuple(gt) if has_gt else ())
        if not all(t.is_cuda and t.device == cols[0].device for t in cols):
            raise ValueError(who + "the columns must be GPU tensors on one device")
        for name, ps in (("lr", lr[2]), ("gt", gt[2] if has_gt else None))[:1 + has_gt]:
            if not bool(((ps == 1) | (ps == -1) | (ps == 0)).all()):
                raise ValueError(who + "%s polarities must be -1, 0 or +1 (counts are integers)" % name)
        self._set_size("open_events", H, W, gh, gw)
        rec = {"lr": tuple(lr), "lr_index": lr_index}
        if has_gt:
            rec.update(gt=tuple(gt), gt_index=gt_index)
        if self.hot_filter is not None:                    # written by bmc_slot_hot_update: the slot is reused after the recording
            from bmc_hip import slots
            _, min_obvs, max_rate = self.hot_filter
            rec.update(hot_pixels=torch.zeros(L - self.seqn + 1, dtype=torch.int32, device=cols[0].device),
                       hot_mask=torch.ones(H, W, dtype=torch.uint8, device=cols[0].device),
                       hot_cmin=[slots.hot_cmin(j + 1, min_obvs, max_rate) for j in range(L)])
        h = self._add(rec, L, cols[0].device, event_capacity, window_event_capacity, spans)
        if not self._has_events:
            self._has_events = True
            self._grow(self._event_buffers)                # a frames-only session: the table grows an event part
        return h

    def resident_bytes(self, handle):
        """Bytes the recording keeps on the GPU: its columns (event-backed) or frames, its result sums, kept predictions and
        (emit_events) its output columns with their index, (voxel_bins=B) its voxel grids: 4 * B * sH * sW bytes per window."""
        r = self._recs[handle]
        data = r["lr"] + r.get("gt", ()) if "lr" in r else (r["frames"],) + ((r["gts"],) if "gts" in r else ())
        if "ev_xs" in r:
            data = tuple(data) + (r["ev_xs"], r["ev_ys"], r["ev_ps"], r["ev_index"]) + ((r["ev_ts"],) if "ev_ts" in r else ())
        data = tuple(data) + ((r["sse"],) if "sse" in r else ()) + (() if r["keep"] is None else (r["keep"],))
        if "hot_pixels" in r:                              # (hot_filter) the per-window mask counts and the last mask
            data = data + (r["hot_pixels"], r["hot_mask"])
        data = data + tuple(r.get("images", {}).values())  # (render) the pictures
        if "voxels" in r:
            data = data + (r["voxels"],)
        return sum(t.numel() * t.element_size() for t in data)

    def scratch_bytes(self):
        """Bytes of the per-slot scratch images of event-backed slots (0 until an event-backed recording has been opened; with
        hot_filter also the slots' counts, mask rings and workspace: 8 + seqn bytes per pixel) and, with event_times, of the
        sort scratch (0 until a recording has been opened); with render, the percentiles and, once a recording with ground truth
        has been opened, the resize scratch [S,2,gh,gw] that bicubic and a resized esr share and the frames [S,2,H,W] it reads;
        with voxel_bins, the partials of the reduce launch (8 bytes per part and slot)."""
        nbytes = 0
        if self.render and self._size is not None:
            nbytes += 4 * 4 * self.S
            if len(self._size) == 4 and self._render_resizes():
                nbytes += 4 * self.S * 2 * (self._size[2] * self._size[3] + ("bicubic" in self.render) * self._size[0] * self._size[1])
        if self._wcap:
            from bmc_hip import slots
            nbytes = slots.emit_timed_scratch_bytes(self.S, self._nparts, self._wcap)
        if self.voxel_bins is not None and self._size is not None:
            nbytes += 4 * 2 * self.S * self._vparts
        if not self._has_events:
            return nbytes
        H, W = self._size[:2]
        gh, gw = self._gt_scratch_size()
        if self.hot_filter is not None:
            nbytes += self.S * H * W * (4 + 4 + self.seqn)
        return nbytes + 4 * self.S * (self.seqn * 2 * H * W + 2 * gh * gw)

    def _gt_scratch_size(self):
        """(gh, gw) of the event-backed slots' ground-truth scratch: a 1 x 1 placeholder (bmc_slot_encode only zero-fills it)
        while no recording of the session has a ground truth."""
        return self._size[2:] if len(self._size) == 4 else (1, 1)

    def results(self, handle):
        """-> dict(esr_mse=[...], bicubic_mse=[...] (a recording with ground truth only), time=[...] per window done so far[,
        hot_pixels=[...] per window, hot_mask=[H,W] uint8 on the GPU (hot_filter, event-backed recordings)][,
        predictions=[n,2,sH,sW]][, images={kind: uint8 [n,h,w,3] on the GPU} (render)][, voxels=[n,B,sH,sW] float32 on the GPU
        (voxel_bins=B)][, sr_events=(xs, ys, ps) of those windows on the GPU, sr_index [done+1] int64 on the host][,
        sr_ts on the GPU, parallel to sr_events (event_times): float32 inside each window, or float64 on the sensor's clock for
        a recording opened with spans / lr_ts]).  Raises RuntimeError when the windows emitted more events than the recording's
        event_capacity, or (event_times) one window more than its window_event_capacity (the message names the capacity
        needed)."""
        r = self._recs[handle]
        done = len(r["steps"])
        if done:
            self._steps[r["steps"][-1]][1].synchronize()
        from bmc_hip import slots
        out = {}
        if "sse" in r:
            sse = slots.sum_parts(r["sse"][:done]) / (2 * self._size[2] * self._size[3])
            out.update(esr_mse=sse[:, 0].tolist(), bicubic_mse=sse[:, 1].tolist())
        out["time"] = [self._steps[k][0].elapsed_time(self._steps[k][1]) for k in r["steps"]]
        if self.keep_predictions:
            out["predictions"] = r["keep"][:done]
        if "hot_pixels" in r:
            out.update(hot_pixels=r["hot_pixels"][:done].tolist(), hot_mask=r["hot_mask"])
        if self.render:
            out["images"] = {k: t[:done] for k, t in r["images"].items()}
        if self.voxel_bins is not None:
            out["voxels"] = r["voxels"][:done]
        if self.emit_events:
            index = r["ev_index"][:done + 1].cpu()
            total = int(index[done])
            if total > r["ev_capacity"]:
                raise RuntimeError("MultiStreamSR.results: recording %d emitted %d events in %d windows, more than its "
                                   "event_capacity of %d: open it with event_capacity >= %d"
                                   % (handle, total, done, r["ev_capacity"], total))
            if self.event_times is not None:
                most = int((index[1:] - index[:-1]).max()) if done else 0
                if most > r["win_capacity"]:
                    raise RuntimeError("MultiStreamSR.results: a window of recording %d emitted %d events, more than its "
                                       "window_event_capacity of %d: open it with window_event_capacity >= %d"
                                       % (handle, most, r["win_capacity"], most))
                out["sr_ts"] = r["ev_ts"][:total]
            out["sr_events"] = (r["ev_xs"][:total], r["ev_ys"][:total], r["ev_ps"][:total])
            out["sr_index"] = index
        return out

    # ---------------------------------------------------------------- windows
    def _buffers(self, device):
        if self._bufs is None:
            H, W = self._size[:2]
            S, nfeat = self.S, 1 if self.plain else 3
            b = {"x": torch.zeros(S, 2, self.seqn, H, W, device=device),
                 "pred": torch.zeros(S, 2, self.scale * H, self.scale * W, device=device)}
            self._new_table(b, device)
            if self.emit_events:
                b["emit_parts"] = torch.zeros(S * self._nparts, dtype=torch.int32, device=device)
            if self.event_times is not None:
                self._sort_buffers(b, device)
            if self._has_events:
                self._event_buffers(b, device)
            self._render_buffers(b, device)
            if self.voxel_bins is not None:
                b["voxel_parts"] = torch.zeros(2 * S * self._vparts, dtype=torch.int32, device=device)
            if self.state_dtype is None:
                b["pool"] = b["feat"] = torch.zeros(nfeat, S, H, W, self.n_c, device=device)       # the model reads the pool
            else:
                b["pool"] = torch.zeros(nfeat, S, H, W, self.n_c, device=device, dtype=self.state_dtype)
                b["feat"] = torch.zeros(nfeat, S, H, W, self.n_c, device=device)
            self._bufs = b
        return self._bufs

    def _new_table(self, b, device):
        """The slot table with the parts the session needs so far."""
        from bmc_hip import slots
        b["table"] = slots.SlotTable(self.S, device, events=self._has_events, emit=self.emit_events,
                                     timed=self.event_times is not None, clock=self._has_clock,
                                     hot=self._has_events and self.hot_filter is not None,
                                     render=len(self.RENDER_TABLES) if self.render else 0,
                                     voxel=self.voxel_bins is not None)

    def _render_resizes(self):
        """Does a session with ground truth resize for its pictures (bicubic always, esr when the sizes differ)?"""
        H, W = self._size[:2]
        return "bicubic" in self.render or ("esr" in self.render and tuple(self._size[2:]) != (self.scale * H, self.scale * W))

    def _render_buffers(self, b, device):
        if not self.render:
            return
        H, W = self._size[:2]
        b["render_minmax"] = torch.zeros(4 * self.S, device=device)
        if len(self._size) == 4 and self._render_resizes():
            b["render_resize"] = torch.zeros(self.S, 2, *self._size[2:], device=device)
            if "bicubic" in self.render:
                b["render_mid"] = torch.zeros(self.S, 2, H, W, device=device)

    def _sort_buffers(self, b, device):
        from bmc_hip import slots
        slots.emit_rank_table(device)                      # uploaded here, once per device: never inside a graph capture
        b["emit_scratch"] = torch.empty(slots.emit_timed_scratch_bytes(self.S, self._nparts, self._wcap), dtype=torch.uint8,
                                        device=device)

    def _gt_scratch(self, b, device):
        if "lr_scratch" in b:                              # (event-backed slots only)
            gh, gw = self._gt_scratch_size()
            b["gt_scratch"] = torch.zeros(self.S, 2, gh, gw, device=device)

    def _event_buffers(self, b, device):
        H, W = self._size[:2]
        if not b["table"].events:
            self._new_table(b, device)
        b["lr_scratch"] = torch.zeros(self.S, self.seqn, 2, H, W, device=device)
        self._gt_scratch(b, device)
        if self.hot_filter is not None:                    # per slot: the running counts, a ring of seqn masks, the workspace
            b["hot_counts"] = torch.zeros(self.S, H, W, dtype=torch.int32, device=device)
            b["hot_ring"] = torch.ones(self.S, self.seqn, H, W, dtype=torch.uint8, device=device)
            b["hot_ws"] = torch.zeros(self.S, H, W, dtype=torch.int32, device=device)

    def _forward(self):
        b = self._bufs
        states = [t.permute(0, 3, 1, 2) for t in b["feat"]]             # channels-last [S,n_c,H,W] views, adjacent
        return self.model(b["x"], *states, b["pred"], False)

    def _window(self):
        """[[hot_update ->] encode ->] stage -> model -> commit [-> metrics] [-> emit] [-> render] [-> voxel] (what a graph replay
        runs)."""
        from bmc_hip import slots
        b = self._bufs
        H, W = self._size[:2]
        if "hot_ring" in b:
            slots.hot_update(b["table"], b["hot_counts"], b["hot_ring"], b["hot_ws"], self.hot_filter[0], self.hot_filter[2])
            slots.encode_filtered(b["table"], b["lr_scratch"], b["gt_scratch"], b["hot_ring"])
        elif "lr_scratch" in b:
            slots.encode(b["table"], b["lr_scratch"], b["gt_scratch"])
        slots.stage(b["table"], b["x"], b["pool"], b["feat"], b["pred"])
        out = self._forward()
        cl = lambda t: t if t.permute(0, 2, 3, 1).is_contiguous() else t.contiguous(memory_format=torch.channels_last)
        slots.commit(b["table"], [cl(t) for t in out[:-1]], b["pool"], out[-1].contiguous(), b["pred"])
        if len(self._size) == 4:                           # a recording with ground truth has been opened
            gh, gw = self._size[2:]
            slots.metrics(b["table"], out[-1].contiguous(), H, W, gh, gw, slots.metric_parts(gh, gw))
        if self.event_times is not None:
            emit = slots.emit_clocked if self._has_clock else slots.emit_timed
            emit(b["table"], out[-1].contiguous(), self.max_count, self._nparts, b["emit_parts"], b["emit_scratch"], self._wcap)
        elif self.emit_events:
            slots.emit(b["table"], out[-1].contiguous(), self.max_count, self._nparts, b["emit_parts"])
        if self.render:
            self._render_window(out[-1].contiguous())
        if self.voxel_bins is not None:
            slots.voxel(b["table"], out[-1].contiguous(), self.max_count, self.voxel_bins, self._vparts, b["voxel_parts"])

    def _render_window(self, pred):
        """The render launches of a window, one pair per table in use: the slots' entries say which of them a slot takes part in.
        The resize scratch serves the resized prediction first and the resized frame 1 after it."""
        from bmc_hip import lib, slots
        from bmc_hip.ops import _stream
        b = self._bufs
        t, mm, S = b["table"], b["render_minmax"], self.S
        H, W = self._size[:2]
        sH, sW = self.scale * H, self.scale * W
        at = self.RENDER_TABLES.index
        if "lr" in self.render:
            slots.render(t, at("lr"), H, W, False, mm)
        if "esr" in self.render:                           # b["pred"]: the window's predictions, where commit has put them
            slots.render(t, at("esr"), sH, sW, True, mm)
        if len(self._size) == 2:
            return
        gh, gw = self._size[2:]
        if "esr" in self.render and (gh, gw) != (sH, sW):
            lib.call(lib._bicubic_fwd, "bmc_bicubic_resize_fwd", pred.data_ptr(), 2 * S, sH, sW, gh, gw,
                     b["render_resize"].data_ptr(), _stream())
            slots.render(t, at("esr_gt"), gh, gw, True, mm)
        if "bicubic" in self.render:
            b["render_mid"].copy_(b["x"][:, :, 1])         # frame 1 of every slot's window, as stage gathered it: [S,2,H,W]
            lib.call(lib._bicubic_fwd, "bmc_bicubic_resize_fwd", b["render_mid"].data_ptr(), 2 * S, H, W, gh, gw,
                     b["render_resize"].data_ptr(), _stream())
            slots.render(t, at("bicubic"), gh, gw, False, mm)
        if "gt" in self.render:
            slots.render(t, at("gt"), gh, gw, False, mm)

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

    def _fill_frames(self, e, r, i):
        """Slot entry e of window i of a frame-backed recording."""
        H, W = self._size[:2]
        e["frames"] = r["frames"].data_ptr() + 4 * i * 2 * H * W
        if "gts" in r:
            e["gt"] = r["gts"].data_ptr() + 4 * (i + 1) * 2 * self._size[2] * self._size[3]

    def _fill_events(self, e, ev, ht, s, r, i, reset):
        """Slot entry e, and entry s of the event (ev) and hot (ht, or None) parts, of window i of an event-backed recording:
        the slot entry points at the slot's scratch images."""
        b = self._bufs
        e["frames"] = b["lr_scratch"][s].data_ptr()
        for k, t in zip(("lr_xs", "lr_ys", "lr_ps", "gt_xs", "gt_ys", "gt_ps"), r["lr"] + r.get("gt", ())):
            ev[k][s] = t.data_ptr()
        ev["lr_range"][s, :self.seqn] = r["lr_index"][i:i + self.seqn]
        if "gt" in r:                                      # (without: NULL columns, range (0, 0): the scratch is only zero-filled)
            e["gt"] = b["gt_scratch"][s].data_ptr()
            ev["gt_range"][s] = r["gt_index"][i + 1]
        if ht is not None:                                 # the first window observes items 0 .. seqn-1, a later one item i+seqn-1
            ht[s]["active"], ht[s]["first_item"], ht[s]["new_from"] = 1, i, 0 if reset else self.seqn - 1
            ht[s]["cmin"][:self.seqn] = r["hot_cmin"][i:i + self.seqn]
            ht[s]["hot_pixels"] = r["hot_pixels"].data_ptr() + 4 * i
            ht[s]["hot_mask"] = r["hot_mask"].data_ptr()

    @staticmethod
    def _fill_emit(em, ck, r, i):
        """Emit entry em and clock entry ck (of a table with a clock part) of window i: it appends at index[i] and leaves
        index[i+1]."""
        em["xs"], em["ys"], em["ps"] = r["ev_xs"].data_ptr(), r["ev_ys"].data_ptr(), r["ev_ps"].data_ptr()
        em["index_in"] = r["ev_index"].data_ptr() + 8 * i
        em["index_out"] = r["ev_index"].data_ptr() + 8 * (i + 1)
        em["capacity"] = r["ev_capacity"]
        if "spans" in r:                                   # window i predicts item i+1: its span, float64 times
            ck["t_first"], ck["t_last"] = r["spans"][i + 1]
            ck["ts"] = r["ev_ts"].data_ptr()
        elif "ev_ts" in r:
            em["ts"] = r["ev_ts"].data_ptr()

    def _fill_render(self, rn, e, s, r, i):
        """Entries s of the render tables rn [K,S] for window i of recording r, whose slot entry e has been filled: where each
        of the recording's pictures reads its count image."""
        b = self._bufs
        H, W = self._size[:2]
        resized = "sse" in r and tuple(self._size[2:]) != (self.scale * H, self.scale * W)
        for kind, img in r["images"].items():
            if kind == "lr":                               # frame 1 of the window
                table, src = "lr", int(e["frames"]) + 4 * 2 * H * W
            elif kind == "esr":
                table, src = ("esr_gt", b["render_resize"][s].data_ptr()) if resized else ("esr", b["pred"][s].data_ptr())
            elif kind == "bicubic":
                table, src = "bicubic", b["render_resize"][s].data_ptr()
            else:
                table, src = "gt", int(e["gt"])
            k = self.RENDER_TABLES.index(table)
            rn[k, s]["src"], rn[k, s]["dst"] = src, img[i].data_ptr()

    def _fill(self, plan):
        """The table entries of the window `plan`, into the table's host copy."""
        from bmc_hip import slots
        t = self._bufs["table"]
        e = t.host()
        ev = t.events_host() if t.events else None
        em = t.emit_host() if self.emit_events else None
        ck = t.clock_host() if t.clock else None
        ht = t.hot_host() if t.hot else None
        vx = t.voxel_host() if t.voxel else None
        for s, p in enumerate(plan):
            if p is None:
                continue
            h, i, reset = p
            r = self._recs[h]
            if "lr" in r:
                self._fill_events(e[s], ev, ht, s, r, i, reset)
            else:
                self._fill_frames(e[s], r, i)
            e[s]["keep"] = r["keep"][i].data_ptr() if r["keep"] is not None else 0
            if "sse" in r:                                 # (without ground truth: gt = 0, result = 0 -- no metrics for the slot)
                e[s]["result"] = r["sse"][i].data_ptr()
            e[s]["flags"] = slots.ACTIVE | (slots.RESET if reset else 0)
            if em is not None:
                self._fill_emit(em[s], ck[s] if "spans" in r else None, r, i)
            if self.render:
                self._fill_render(t.render_host(), e[s], s, r, i)
            if vx is not None:
                vx[s]["dst"] = r["voxels"][i].data_ptr()
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
                        window_event_capacity=None, hot_filter=None, render=None, voxel_bins=None):
    """infer_BMCNet.py mode 1 (:248-295) through MultiStreamSR: recordings = {name: (frames [L,2,H,W], gts [L,2,gh,gw])}
    (or a sequence of such pairs, named "0", "1", ...) of one sensor size; an item may also be an EventRecording (raw event
    columns + index tables, encoded window by window: MultiStreamSR.open_events).  A recording WITHOUT ground truth is
    (frames, None) or an EventRecording with gt = None.  -> dict(
      results = {metric: {name: value}}  per recording the mean over its windows of esr_mse, bicubic_mse (recordings with
                                         ground truth only), time (ms), and params (millions) -- infer_body's MetricTracker
                                         result (:34,:70-86),
      mean    = {metric: mean over the recordings listed}  (results_mean, :284-291; a metric no recording has is absent)[,
      predictions = {name: [n_windows,2,sH,sW]}  with keep_predictions][,
      sr_events   = {name: (xs, ys, ps, index [n_windows+1])}  with emit_events: the super-resolved event stream of every
                                         recording (MultiStreamSR(emit_events=True); event_capacity: per recording, None =
                                         the default)][,
      sr_ts       = {name: ts float32}           with event_times="linear": the events' times inside their windows, every
                                         window in time order (window_event_capacity: per recording, None = the default)]).
      images      = {name: {kind: uint8 [n_windows,h,w,3]}}  with render: the event-count images of every recording]).
    hot_filter: MultiStreamSR's option (the EventRecording items are filtered, frame pairs are not).  render: MultiStreamSR's
    option (a tuple of kinds from "lr", "bicubic", "esr", "gt").  voxel_bins=B: MultiStreamSR's option; the result then carries
    voxels = {name: float32 [n_windows,B,sH,sW]}."""
    items = list(recordings.items()) if isinstance(recordings, dict) else [(str(i), r) for i, r in enumerate(recordings)]
    ms = MultiStreamSR(model, slots, n_c=n_c, scale=scale, plain=plain, graph=graph, state_dtype=state_dtype,
                       keep_predictions=keep_predictions, seqn=seqn, emit_events=emit_events, max_count=max_count, event_times=event_times,
                       hot_filter=hot_filter, render=render, voxel_bins=voxel_bins)
    handles = []
    for name, r in items:
        if isinstance(r, EventRecording):
            if gt_size is not None and r.gt_size is not None and tuple(int(v) for v in gt_size) != tuple(int(v) for v in r.gt_size):
                raise ValueError("evaluate_recordings: gt_size %s differs from recording %s's %s"
                                 % (tuple(gt_size), name, tuple(r.gt_size)))
            handles.append((name, ms.open_events(*r, event_capacity=event_capacity,
                                                 window_event_capacity=window_event_capacity)))
        else:
            handles.append((name, ms.open(r[0], r[1], gt_size if r[1] is not None else None, event_capacity=event_capacity,
                                          window_event_capacity=window_event_capacity)))
    ms.run()
    params = sum(p.numel() for p in model.parameters()) / 1e6
    breakdown = {k: {} for k in ("esr_mse", "bicubic_mse", "time", "params")}
    preds, streams, times, images, voxels = {}, {}, {}, {}, {}
    for name, h in handles:
        r = ms.results(h)
        for k in ("esr_mse", "bicubic_mse", "time"):
            if k in r:
                breakdown[k][name] = float(statistics.mean(r[k]))
        breakdown["params"][name] = params
        if keep_predictions:
            preds[name] = r["predictions"]
        if emit_events:
            streams[name] = r["sr_events"] + (r["sr_index"],)
        if event_times is not None:
            times[name] = r["sr_ts"]
        if ms.render:
            images[name] = r["images"]
        if ms.voxel_bins is not None:
            voxels[name] = r["voxels"]
    out = {"results": breakdown, "mean": {k: float(statistics.mean(v.values())) for k, v in breakdown.items() if v}}
    if keep_predictions:
        out["predictions"] = preds
    if emit_events:
        out["sr_events"] = streams
    if event_times is not None:
        out["sr_ts"] = times
    if ms.render:
        out["images"] = images
    if ms.voxel_bins is not None:
        out["voxels"] = voxels
    return out
