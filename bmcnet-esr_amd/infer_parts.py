"""The parts of infer.MultiStreamSR: one small class per option of a session, holding everything the session does for it.

A part works on the session's own dicts -- ms._bufs (the session's buffers), ms._recs[h] (a recording) -- and on its sizes; it is a
way to group code, not a data model: a part keeps nothing itself, every hook takes the session `ms` first (left out below).  The
session keeps its parts in the launch order of a window and loops over them:

  table()                    the keywords slots.SlotTable needs for the part now
  open(rec, L, ...)          a recording of L items is opened: checks, and the tensors the part adds to the record; nothing of the
                             session changes here, so a refused recording leaves no trace
  grew(rec)                  the recording is accepted: note what it is the first to bring (an event-backed or clocked recording,
                             a larger window capacity) -> True when the part's buffers or table keywords changed
  scratch()                  {key: (shape, dtype, fill, counted)}: the part's buffers in ms._bufs at the session's current sizes
                             (fill None: uninitialised); the session allocates from it, scratch_bytes() sums its counted entries
  fill(v, s, r, i, reset)    the part's table entries for slot s running window i of record r; v: the host views of the table's
                             sections by name ("slot", "events", "emit", "clock", "hot", "render", "voxel", "quality")
  launch(b, pred)            the part's launches of a window on b = ms._bufs; input parts run before bmc_slot_stage (pred None),
                             the others after bmc_slot_commit with the window's prediction
  results(out, r, done, h)   the part's keys of results(h) after `done` windows, and its capacity errors"""
import numpy as np
import torch

from bmc_hip import lib, slots, stream_lib
from bmc_hip.encodings import check_spans
from bmc_hip.ops import _stream

F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8


class Part:
    """What a part that overrides nothing answers: no keyword, no buffer, no entry, no launch, no key, never grown."""
    input = False                # an input part launches before bmc_slot_stage
    table = scratch = lambda self, ms: {}
    open = grew = fill = launch = results = lambda self, ms, *args, **room: None


class HotFilter(Part):
    """hot_filter=dict(max_px=, min_obvs=, max_rate=): the reference's hot-pixel filter (dataset.hot_filter; create_hot_mask,
    dataloader/h5dataset.py:528-548; get_hot_event_mask, dataloader/encodings.py:349-364) on the GPU, for recordings opened with
    open_events: every LR item is observed once, in item order (a per-slot count of the items in which a pixel fired), its mask
    follows the reference's rule bit for bit, and the item's count image has both channels zeroed where the mask says so --
    include/bmc_hip.h states the contract.  bmc_slot_hot_update (one more launch per window for all slots, inside the captured
    graph too) runs before the encode launch, which becomes bmc_slot_encode_filtered.  Recordings opened with open() in the same
    session stay UNFILTERED, and so does every ground truth.  results() then carries hot_pixels (per window, the number of
    pixels masked for the item that window newly observed) and hot_mask ([H,W] uint8 in sensor coordinates, 1 = kept, of the
    last item observed).  Per slot: the running counts, a ring of seqn masks and the workspace, 8 + seqn bytes per pixel.  The
    option needs nothing else switched on."""
    input = True

    def table(self, ms):
        return {"hot": ms._has_events}

    def open(self, ms, rec, L, **room):
        if "lr" not in rec:
            return
        who = "MultiStreamSR.open_events: "
        if L >= slots.HOT_MAX_ITEMS:
            raise ValueError(who + "a filtered session takes recordings of fewer than 2^23 items (got %d)" % L)
        if int((rec["lr_index"][:, 1] - rec["lr_index"][:, 0]).max()) >= 2 ** 31:
            raise ValueError(who + "a filtered session takes LR items of fewer than 2^31 events")
        _, min_obvs, max_rate = ms.hot_filter              # written by bmc_slot_hot_update: the slot is reused after the recording
        rec.update(hot_pixels=torch.zeros(rec["n"], dtype=I32, device=rec["device"]),
                   hot_mask=torch.ones(*ms._size[:2], dtype=U8, device=rec["device"]),
                   hot_cmin=[slots.hot_cmin(j + 1, min_obvs, max_rate) for j in range(L)])

    def scratch(self, ms):
        if not ms._has_events:
            return {}
        H, W = ms._size[:2]
        return {"hot_counts": ((ms.S, H, W), I32, 0, True), "hot_ring": ((ms.S, ms.seqn, H, W), U8, 1, True),
                "hot_ws": ((ms.S, H, W), I32, 0, True)}

    def fill(self, ms, v, s, r, i, reset):
        if "lr" in r:                                      # the first window observes items 0 .. seqn-1, a later one item i+seqn-1
            ht, seqn = v["hot"][s], ms.seqn
            ht["active"], ht["first_item"], ht["new_from"] = 1, i, 0 if reset else seqn - 1
            ht["cmin"][:seqn] = r["hot_cmin"][i:i + seqn]
            ht["hot_pixels"] = r["hot_pixels"].data_ptr() + 4 * i
            ht["hot_mask"] = r["hot_mask"].data_ptr()

    def launch(self, ms, b, pred):
        if "hot_ring" in b:
            slots.hot_update(b["table"], b["hot_counts"], b["hot_ring"], b["hot_ws"], ms.hot_filter[0], ms.hot_filter[2])

    def results(self, ms, out, r, done, handle):
        if "hot_pixels" in r:
            out.update(hot_pixels=r["hot_pixels"][:done].tolist(), hot_mask=r["hot_mask"])


class Input(Part):
    """Where a slot's frames come from.  A frame-backed recording (open) points the slot at its own frames and ground truth.  An
    EVENT-BACKED one (open_events) keeps the raw dataset columns on the GPU (12 bytes per event instead of 8 bytes per pixel of
    every frame) and the frames of a window are encoded on the fly by bmc_slot_encode -- one more launch per window for all
    slots, into per-slot scratch that the slot's table entry points at; the other kernels do not know the difference, and the
    results are bit-identical to open() on the frames the raw-column encoder (ops.encode_raw_events, no flips) gives for the same
    ranges.  The encode launch is issued only once an event-backed recording has been opened (the first after a capture
    invalidates the graph); both kinds may share a session.  While no recording has a ground truth the ground-truth scratch is a
    1 x 1 placeholder (bmc_slot_encode only zero-fills it)."""
    input = True

    def table(self, ms):
        return {"events": ms._has_events}

    def grew(self, ms, rec):
        first = "lr" in rec and not ms._has_events
        ms._has_events |= first
        return first

    def scratch(self, ms):
        if not ms._has_events:
            return {}
        gh, gw = ms._size[2:] if len(ms._size) == 4 else (1, 1)
        return {"lr_scratch": ((ms.S, ms.seqn, 2) + tuple(ms._size[:2]), F32, 0, True), "gt_scratch": ((ms.S, 2, gh, gw), F32, 0, True)}

    def fill(self, ms, v, s, r, i, reset):
        e = v["slot"][s]
        H, W = ms._size[:2]
        if "lr" not in r:
            e["frames"] = r["frames"].data_ptr() + 4 * i * 2 * H * W
            if "gts" in r:
                e["gt"] = r["gts"].data_ptr() + 4 * (i + 1) * 2 * ms._size[2] * ms._size[3]
            return
        b, ev = ms._bufs, v["events"]                      # the slot entry points at the slot's scratch images
        e["frames"] = b["lr_scratch"][s].data_ptr()
        for k, t in zip(("lr_xs", "lr_ys", "lr_ps", "gt_xs", "gt_ys", "gt_ps"), r["lr"] + r.get("gt", ())):
            ev[k][s] = t.data_ptr()
        ev["lr_range"][s, :ms.seqn] = r["lr_index"][i:i + ms.seqn]
        if "gt" in r:                                      # (without: NULL columns, range (0, 0): the scratch is only zero-filled)
            e["gt"] = b["gt_scratch"][s].data_ptr()
            ev["gt_range"][s] = r["gt_index"][i + 1]

    def launch(self, ms, b, pred):
        if "hot_ring" in b:
            slots.encode_filtered(b["table"], b["lr_scratch"], b["gt_scratch"], b["hot_ring"])
        elif "lr_scratch" in b:
            slots.encode(b["table"], b["lr_scratch"], b["gt_scratch"])


class Metrics(Part):
    """esr_mse / bicubic_mse per window of a recording WITH ground truth (bmc_slot_metrics: sums per slot, read only when results()
    asks).  A recording without one (open(frames), open_events(lr, None, lr_index, None, lr_size)) is what a deployed sensor
    delivers: its results() carry no metric, it only has to match the session's (H, W) and may share it with recordings that
    have a ground truth.  bmc_slot_metrics is launched only once a recording with ground truth has been opened (the first such
    open after a capture invalidates the graph)."""

    def open(self, ms, rec, L, **room):
        if "gts" in rec or "gt" in rec:
            rec["sse"] = torch.zeros(rec["n"], slots.metric_parts(*ms._size[2:]), 2, dtype=torch.float64, device=rec["device"])

    def fill(self, ms, v, s, r, i, reset):
        if "sse" in r:                                     # (without ground truth: gt = 0, result = 0 -- no metrics for the slot)
            v["slot"][s]["result"] = r["sse"][i].data_ptr()

    def launch(self, ms, b, pred):
        if len(ms._size) == 4:                             # a recording with ground truth has been opened
            slots.metrics(b["table"], pred, *ms._size, slots.metric_parts(*ms._size[2:]))

    def results(self, ms, out, r, done, handle):
        if "sse" in r:
            sse = slots.sum_parts(r["sse"][:done]) / (2 * ms._size[2] * ms._size[3])
            out.update(esr_mse=sse[:, 0].tolist(), bicubic_mse=sse[:, 1].tolist())


class Quality(Part):
    """quality=True or dict(data_range="gt" | R): esr_psnr, esr_ssim, bicubic_psnr, bicubic_ssim per window of a recording WITH
    ground truth -- the other two columns of a super-resolution table, the reference's psnr_loss / ssim_loss (loss/restore.py:44-93:
    scikit-image's peak_signal_noise_ratio and structural_similarity per channel on the CPU, after a .cpu().numpy() of every
    prediction), computed on the GPU in float64 (bmc_slot_quality: three more launches per window for all slots, inside the captured
    graph too; no atomics, no host sync; include/bmc_hip_quality.h states the contract).  Per channel c of the two-channel count
    image, then the mean of the two: PSNR = 10 log10(R_c^2 / mse_c); SSIM with a uniform 7x7 window, K1 = 0.01, K2 = 0.03 and
    sample covariance, averaged over the (gh - 6) x (gw - 6) window positions inside the image.  R_c = max(gt[c]) - min(gt), the
    minimum over both channels (restore.py:85), or the constant R.  IEEE results stand: +inf PSNR for an exact channel, -inf for
    R_c = 0 with an error; SSIM is nan for R_c = 0.  "esr" is the window's prediction (the MERGED one in a self-ensemble session,
    as esr_mse), "bicubic" frame 1 of the window as the model saw it (after the hot-pixel filter where one applies); both are
    resized to the ground truth's size with bmc_bicubic_resize_fwd where theirs differs -- the float32 values esr_mse and the
    pictures use.  The error is subtracted in float64 here and in float32 in esr_mse, so esr_psnr is not a function of esr_mse
    to the last bit.  A ground truth must be at least 7 x 7 (ValueError at open).  Resident: 128 bytes per window; session
    scratch once a recording with ground truth has been opened: the bicubic baseline [S,2,gh,gw], the resized prediction (the
    same again) where sizes differ, frame 1 [S,2,H,W], and the partial sums of the launches.  A recording without ground truth
    carries none of the keys; bmc_slot_quality is launched only once a recording with ground truth has been opened."""
    KEYS = ("esr_psnr", "esr_ssim", "bicubic_psnr", "bicubic_ssim")

    @staticmethod
    def check(who, quality):
        """quality (None, True, or a dict with exactly the key data_range: "gt" or a finite positive number) -> None or the data
        range ("gt" or a float); ValueError otherwise."""
        if quality is None:
            return None
        if quality is True:
            return "gt"
        if not isinstance(quality, dict):
            raise ValueError(who + "quality must be None, True or a dict with the key data_range (got %r)" % (quality,))
        for k in quality:
            if k != "data_range":
                raise ValueError(who + "quality has an unknown key %r (the key is data_range)" % (k,))
        if "data_range" not in quality:
            raise ValueError(who + "quality lacks the key 'data_range'")
        rng = slots.check_data_range(who + "quality: ", quality["data_range"])
        return "gt" if rng == 0.0 else rng

    @staticmethod
    def check_size(who, gh, gw):
        """The ground truth of a recording a session with quality takes: at least one window position."""
        if min(gh, gw) < slots.QUALITY_WIN:
            raise ValueError("MultiStreamSR.%s: quality needs a ground truth of at least %d x %d (got %d x %d)"
                             % (who, slots.QUALITY_WIN, slots.QUALITY_WIN, gh, gw))

    def table(self, ms):
        return {"quality": True}

    def open(self, ms, rec, L, **room):
        if "sse" in rec:                                   # (Metrics, the part before: the recording has a ground truth)
            rec["quality"] = torch.zeros(rec["n"], 2, 2, slots.QUALITY_WORDS, dtype=F64, device=rec["device"])

    def scratch(self, ms):
        if len(ms._size) != 4:
            return {}
        S, (H, W, gh, gw) = ms.S, ms._size
        d = {"quality_stats": ((S, slots.metric_parts(gh, gw), slots.QUALITY_STATS_WORDS), F64, 0, True),
             "quality_tiles": ((S, 4, slots.quality_tiles(gh, gw)), F64, 0, True),
             "quality_resize": ((S, 2, gh, gw), F32, 0, True), "quality_mid": ((S, 2, H, W), F32, 0, True)}
        if (gh, gw) != (ms.scale * H, ms.scale * W):
            d["quality_resize_esr"] = ((S, 2, gh, gw), F32, 0, True)
        return d

    def fill(self, ms, v, s, r, i, reset):
        if "quality" in r:                                 # (without ground truth: dst = 0 -- no record for the slot)
            v["quality"][s]["dst"] = r["quality"][i].data_ptr()

    def launch(self, ms, b, pred):
        if len(ms._size) != 4:                             # no recording with ground truth yet
            return
        S, (H, W, gh, gw) = ms.S, ms._size
        esr = pred                                         # (a self-ensemble session: the merged prediction is in the leader's row)
        if "quality_resize_esr" in b:
            esr = b["quality_resize_esr"]
            lib.call(lib._bicubic_fwd, "bmc_bicubic_resize_fwd", pred.data_ptr(), 2 * S, ms.scale * H, ms.scale * W, gh, gw,
                     esr.data_ptr(), _stream())
        b["quality_mid"].copy_(b["x"][:, :, 1])            # frame 1 of every slot's window, as stage gathered it: [S,2,H,W]
        lib.call(lib._bicubic_fwd, "bmc_bicubic_resize_fwd", b["quality_mid"].data_ptr(), 2 * S, H, W, gh, gw,
                 b["quality_resize"].data_ptr(), _stream())
        slots.quality(b["table"], esr, b["quality_resize"], slots.metric_parts(gh, gw), 0.0 if ms.quality == "gt" else ms.quality,
                      b["quality_stats"], b["quality_tiles"])

    def results(self, ms, out, r, done, handle):
        if "quality" in r:
            psnr, ssim = slots.quality_values(r["quality"][:done], ms.quality, ms._size[2:])       # [done, 2 images] each
            out.update(esr_psnr=psnr[:, 0].tolist(), esr_ssim=ssim[:, 0].tolist(), bicubic_psnr=psnr[:, 1].tolist(),
                       bicubic_ssim=ssim[:, 1].tolist())


class KeptPredictions(Part):
    """keep_predictions: results() carries predictions [n_windows,2,sH,sW], written by bmc_slot_commit (8 x sH x sW bytes each)."""

    def open(self, ms, rec, L, **room):
        rec["keep"] = torch.empty(rec["n"], 2, ms.scale * ms._size[0], ms.scale * ms._size[1], device=rec["device"])

    def fill(self, ms, v, s, r, i, reset):
        v["slot"][s]["keep"] = r["keep"][i].data_ptr()

    def results(self, ms, out, r, done, handle):
        out["predictions"] = r["keep"][:done]


class EventStream(Part):
    """emit_events=True: every window's prediction is also turned into an EVENT LIST on the GPU (bmc_slot_emit: two more launches
    per window for all slots, inside the captured graph too) and appended to the recording's own output columns: per element v
    of the prediction [2,sH,sW] in flat order, q = min(rint(v), max_count) for v > 0 (else 0; round-half-to-even -- the rounded
    count image the reference renders, infer_BMCNet.py:94) events xs = x, ys = sH-1-row, ps = +1 (channel 0) / -1 (channel 1),
    so that encoding a window's events at (sH, sW) gives q back exactly.  results() then carries sr_events = (xs int16, ys int16,
    ps int8) and sr_index [done+1] (window i owns events [sr_index[i], sr_index[i+1])); without event_times there are no
    timestamps and a window's events are in pixel order.  The columns hold `event_capacity` events (open / open_events; default
    2 x scale^2 x the recording's LR events); the index keeps counting past it, and results() then raises with the capacity that
    is needed.  About 5 bytes per event instead of 8 x sH x sW bytes per window of keep_predictions; both may be on.

    event_times="linear" (with emit_events; needs max_count <= 255): the list becomes a STREAM.  Every event also carries a
    float32 time inside its window and a window's events are stored in time order (bmc_slot_emit_timed: six launches per
    window instead of the two, inside the captured graph too) -- the reference's linear redistribution of a count image
    (dataloader/encodings.py:367-414, mode='linear', one time bin): event j of a pixel's n events has t = 0.01 + 0.99 * j /
    (n - 1) (0.01 for n = 1; float64, rounded once), the window is sorted by the exact j / (n - 1), ties in the pixel order
    above.  results() then also carries sr_ts (float32, on the GPU), parallel to sr_events.  Times are window-normalised: a
    count image has no absolute clock.  The sort works in per-slot scratch of `window_event_capacity` events (open /
    open_events; default 2 x scale^2 x the LR events of the recording's busiest frame, at most 2 x sH x sW x max_count); a
    window that emits more stores nothing, the index keeps the true count and results() raises with the capacity needed.

    Events on the SENSOR'S CLOCK (event_times="linear"; open(..., spans=) / open_events(..., lr_ts= or spans=)): spans [L,2]
    float64 = (t_first, t_last) of every item on the recording's own time base (open_events derives them from the timestamp
    column lr_ts: bmc_hip.encodings.event_block_spans).  Window i predicts item i+1 (infer_BMCNet.py:52) and uses its span:
    sr_ts is then FLOAT64, t = t_first + tau * (t_last - t_first) with tau the window time above computed from the reduced
    fraction of j / (n - 1) (bmc_slot_emit_clocked; include/bmc_hip.h states the contract) -- the inverse of
    event_formatting's normalisation (dataloader/base_dataset.py:30) without its 1e-6.  Each window is in time order; with
    sliding_window < window the spans of consecutive windows overlap, so the concatenation of a recording's windows carries
    every stretch of sensor time as often as items cover it and is not in time order -- unless the session is continuous
    (below).  Clocked and unclocked recordings may share a session; the first clocked
    one adds the table's clock section, a larger window_event_capacity a larger sort scratch (either invalidates the graph).

    ONE CONTINUOUS STREAM (continuous=True; needs event_times="linear", and every recording spans / lr_ts): window i, which
    predicts item i+1, emits only its events with t < t_cut = spans[i+2][0], the start of the item the next window predicts
    (+inf for the recording's last window): bmc_slot_emit_trimmed, include/bmc_hip_stream.h states the contract.  The kept
    events are a prefix of the window's sorted events with the same bytes, found BEFORE the sort (the same six launches), so
    sr_events / sr_ts of a recording are globally non-decreasing in time and cover every instant once; with spans that do not
    overlap nothing is dropped and every byte equals the option off.  sr_index, event_capacity and window_event_capacity
    count KEPT events; results() also carries sr_dropped, the events every window lost to its cut (written by the kernel: no
    host sync).  The t_first column of the spans must not decrease over the items the windows predict.

    The part is in every session: without emit_events it only refuses the arguments that need it."""

    @staticmethod
    def check(emit_events, event_times, max_count, continuous=False):
        if event_times not in (None, "linear"):
            raise ValueError("MultiStreamSR: event_times must be None or 'linear' (got %r)" % (event_times,))
        if event_times is not None and not emit_events:
            raise ValueError("MultiStreamSR: event_times needs emit_events=True")
        if event_times is not None and max_count > slots.MAX_COUNT_TIMED:
            raise ValueError("MultiStreamSR: event_times needs max_count <= %d (got %d)" % (slots.MAX_COUNT_TIMED, max_count))
        if not isinstance(continuous, (bool, np.bool_)):
            raise ValueError("MultiStreamSR: continuous must be True or False (got %r)" % (continuous,))
        if continuous and event_times != "linear":
            raise ValueError("MultiStreamSR: continuous=True needs event_times='linear' (the cut is made on the events' clock)")

    def table(self, ms):
        return {"emit": ms.emit_events, "timed": ms.event_times is not None, "clock": ms._has_clock,
                "trim": ms.continuous and ms._has_clock}

    # the checks of open / open_events: methods of their own, because they come before those of the recording's tensors
    def check_capacities(self, ms, who, event_capacity, capacity):
        """The two capacities a caller of open / open_events may give (None: the default)."""
        if event_capacity is not None:
            if not ms.emit_events:
                raise ValueError("MultiStreamSR.%s: event_capacity needs a session with emit_events=True" % who)
            if isinstance(event_capacity, bool) or not isinstance(event_capacity, (int, np.integer)) or event_capacity < 1:
                raise ValueError("MultiStreamSR.%s: event_capacity must be a positive integer (got %r)" % (who, event_capacity))
        if capacity is not None:
            if ms.event_times is None:
                raise ValueError("MultiStreamSR.%s: window_event_capacity needs a session with event_times='linear'" % who)
            if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not 1 <= capacity <= slots.MAX_WINDOW_CAPACITY:
                raise ValueError("MultiStreamSR.%s: window_event_capacity must be a positive integer, at most %d (got %r)"
                                 % (who, slots.MAX_WINDOW_CAPACITY, capacity))

    def check_spans(self, ms, who, spans, L=None):
        """spans (or None) -> a validated [L,2] float64 table on the host (or None); L None: only that the session takes spans."""
        if spans is None:
            if ms.continuous:
                raise ValueError("MultiStreamSR.%s: a continuous session needs spans / lr_ts of every recording (there is no "
                                 "clock to cut on)" % who)
            return None
        if ms.event_times is None:
            raise ValueError("MultiStreamSR.%s: spans / lr_ts need a session with event_times='linear'" % who)
        if L is None:
            return spans
        spans = check_spans("MultiStreamSR.%s: " % who, spans, L)
        if ms.continuous and (np.diff(spans[1:L - ms.seqn + 2, 0]) < 0).any():      # windows 0 .. n-1 predict items 1 .. n
            raise ValueError("MultiStreamSR.%s: a continuous session needs spans whose t_first does not decrease over the "
                             "items the windows predict" % who)
        return spans

    @staticmethod
    def cuts(spans, n):
        """[n] float64: the cut of every window of a recording with these spans -- window i predicts item i+1 and is cut at
        spans[i+2][0], the start of the item the next window predicts; the last window (or i+2 >= L) at +inf."""
        cuts = np.full(n, np.inf)
        k = max(min(n - 1, len(spans) - 2), 0)
        cuts[:k] = spans[2:2 + k, 0]
        return cuts

    def room(self, ms, who, H, W, event_capacity, window_event_capacity, total, busiest):
        """What an emitting session needs of a recording of H x W frames: coordinates in int16, and the two capacities (defaults:
        the class docstring's).  total / busiest give the recording's counts and are called only where a default is needed."""
        if ms.emit_events and max(ms.scale * H, ms.scale * W) > slots.MAX_COUNT_LIMIT:
            raise ValueError("MultiStreamSR.%s: predictions of %d x %d cannot be emitted (int16 coordinates)"
                             % (who, ms.scale * H, ms.scale * W))
        if ms.emit_events and event_capacity is None:
            event_capacity = 2 * ms.scale ** 2 * int(total())
        if ms.event_times is not None and window_event_capacity is None:
            most = 2 * ms.scale ** 2 * H * W * ms.max_count
            window_event_capacity = max(1, min(2 * ms.scale ** 2 * int(busiest()), most, slots.MAX_WINDOW_CAPACITY))
        return event_capacity, window_event_capacity

    def open(self, ms, rec, L, event_capacity=None, window_event_capacity=None, spans=None):
        if not ms.emit_events:
            return
        cap, device = max(int(event_capacity), 1), rec["device"]      # the output stream: three columns and the index table
        column = lambda dtype: torch.empty(cap, dtype=dtype, device=device)
        rec.update(ev_capacity=cap, ev_xs=column(torch.int16), ev_ys=column(torch.int16), ev_ps=column(torch.int8),
                   ev_index=torch.zeros(rec["n"] + 1, dtype=torch.int64, device=device))
        if ms.event_times is not None:                     # ... a time column, and room for its largest window in the sort
            slots.emit_rank_table(device)                  # uploaded here, once per device: never inside a graph capture
            rec.update(ev_ts=column(F32 if spans is None else torch.float64), win_capacity=int(window_event_capacity))
            if spans is not None:                          # a clocked recording: float64 times on its own clock
                rec["spans"] = spans
            if ms.continuous:                              # (its spans were demanded at the door) the cuts, the dropped counts
                rec.update(cuts=self.cuts(spans, rec["n"]), ev_dropped=torch.zeros(rec["n"], dtype=torch.int64, device=device))

    def grew(self, ms, rec):
        clock, room = "spans" in rec and not ms._has_clock, rec.get("win_capacity", 0) > ms._wcap
        ms._has_clock |= clock
        ms._wcap = max(ms._wcap, rec.get("win_capacity", 0))
        return clock or room

    def scratch(self, ms):
        if not ms.emit_events:
            return {}
        words = stream_lib.TRIM_PARTS if ms.continuous else 1             # (a trimmed count launch: kept and dropped totals)
        d = {"emit_parts": ((words * ms.S * ms._nparts,), I32, 0, False)}  # (scratch_bytes() never counted the count launch's totals)
        if ms._wcap:
            d["emit_scratch"] = ((slots.emit_timed_scratch_bytes(ms.S, ms._nparts, ms._wcap),), U8, None, True)
        return d

    def fill(self, ms, v, s, r, i, reset):
        if "ev_xs" not in r:
            return
        em = v["emit"][s]                                  # window i appends at index[i] and leaves index[i+1]
        em["xs"], em["ys"], em["ps"] = r["ev_xs"].data_ptr(), r["ev_ys"].data_ptr(), r["ev_ps"].data_ptr()
        em["index_in"], em["index_out"] = r["ev_index"].data_ptr() + 8 * i, r["ev_index"].data_ptr() + 8 * (i + 1)
        em["capacity"] = r["ev_capacity"]
        if "spans" in r:                                   # window i predicts item i+1: its span, float64 times
            ck = v["clock"][s]
            ck["t_first"], ck["t_last"] = r["spans"][i + 1]
            ck["ts"] = r["ev_ts"].data_ptr()
            if "cuts" in r:                                # a continuous session: the events before the next window's item
                tr = v["trim"][s]
                tr["t_cut"], tr["dropped"] = r["cuts"][i], r["ev_dropped"].data_ptr() + 8 * i
        elif "ev_ts" in r:
            em["ts"] = r["ev_ts"].data_ptr()

    def launch(self, ms, b, pred):
        if ms.event_times is not None:
            emit = slots.emit_trimmed if ms.continuous else slots.emit_clocked if ms._has_clock else slots.emit_timed
            emit(b["table"], pred, ms.max_count, ms._nparts, b["emit_parts"], b["emit_scratch"], ms._wcap)
        elif ms.emit_events:
            slots.emit(b["table"], pred, ms.max_count, ms._nparts, b["emit_parts"])

    def results(self, ms, out, r, done, handle):
        if "ev_xs" not in r:
            return
        index = r["ev_index"][:done + 1].cpu()
        total = int(index[done])
        if total > r["ev_capacity"]:
            raise RuntimeError("MultiStreamSR.results: recording %d emitted %d events in %d windows, more than its "
                               "event_capacity of %d: open it with event_capacity >= %d"
                               % (handle, total, done, r["ev_capacity"], total))
        if "ev_ts" in r:
            most = int((index[1:] - index[:-1]).max()) if done else 0
            if most > r["win_capacity"]:
                raise RuntimeError("MultiStreamSR.results: a window of recording %d emitted %d events, more than its "
                                   "window_event_capacity of %d: open it with window_event_capacity >= %d"
                                   % (handle, most, r["win_capacity"], most))
            out["sr_ts"] = r["ev_ts"][:total]
        if "ev_dropped" in r:
            out["sr_dropped"] = r["ev_dropped"][:done].tolist()
        out["sr_events"] = (r["ev_xs"][:total], r["ev_ys"][:total], r["ev_ps"][:total])
        out["sr_index"] = index


class Pictures(Part):
    """render=(kinds...) from ("lr", "bicubic", "esr", "gt"): the four EVENT-COUNT IMAGES the reference's inference writes per
    window (infer_BMCNet.py:90-97: lr_event_img, hr_bicubic_event_img, hr_esr_event_img, hr_gt_event_img), rendered on the GPU as
    the uint8 [h,w,3] arrays its plot_event_cnt returns, byte for byte (bmc_slot_render: two launches per kind for all slots,
    inside the captured graph too; include/bmc_hip.h "event-count images" states the contract).  lr: frame 1 of the window as
    the model sees it (H x W; after the hot-pixel filter where one applies); esr: the prediction, resized to the ground truth's
    size where that differs (bmc_bicubic_resize_fwd, as the metric does) and rounded half-to-even; bicubic: frame 1 resized to
    the ground truth's size; gt: the window's ground truth.  A recording without ground truth gets lr and esr (at the
    prediction's size) only.  results() then carries images = {kind: uint8 [done,h,w,3]} on the GPU: 3 bytes per pixel and
    window instead of the 8 of keep_predictions.  Session buffers: the percentiles and, once a recording with ground truth has
    been opened, the resize scratch [S,2,gh,gw] that bicubic and a resized esr share and the frames [S,2,H,W] bicubic reads."""
    KINDS = ("lr", "bicubic", "esr", "gt")
    # the render tables of the slot table: "esr" draws from the prediction, "esr_gt" from the prediction resized to the ground truth
    TABLES = ("lr", "esr", "esr_gt", "bicubic", "gt")

    @staticmethod
    def check(who, render):
        """render (None, or a tuple / list of distinct kinds from KINDS) -> the kinds in KINDS' order (() for None), or ValueError."""
        if render is None:
            return ()
        if isinstance(render, str) or not isinstance(render, (tuple, list)) or not render:
            raise ValueError(who + "render must be None or a non-empty tuple of kinds from %s (got %r)" % (Pictures.KINDS, render))
        for k in render:
            if not isinstance(k, str) or k not in Pictures.KINDS:
                raise ValueError(who + "render has an unknown kind %r (the kinds are %s)" % (k, ", ".join(Pictures.KINDS)))
        if len(set(render)) != len(render):
            raise ValueError(who + "render names a kind twice (got %r)" % (render,))
        return tuple(k for k in Pictures.KINDS if k in render)

    def table(self, ms):
        return {"render": len(self.TABLES)}

    def size(self, ms, kind, has_gt):
        """(h, w) of a recording's image of `kind`."""
        H, W = ms._size[:2]
        if kind == "lr":
            return H, W
        return tuple(ms._size[2:]) if has_gt else (ms.scale * H, ms.scale * W)

    def tables(self, ms):
        """[(render table, h, w, round)] of the session's render launches, in launch order: the slots' entries say which of them
        a slot takes part in.  With a ground truth: esr_gt where its size differs from the prediction's, bicubic, gt."""
        kinds, has_gt = ms.render, len(ms._size) == 4
        lr, sr, gt = self.size(ms, "lr", False), self.size(ms, "esr", False), self.size(ms, "gt", has_gt)
        use = [("lr", lr, False, "lr" in kinds), ("esr", sr, True, "esr" in kinds), ("esr_gt", gt, True, "esr" in kinds and has_gt and gt != sr),
               ("bicubic", gt, False, "bicubic" in kinds and has_gt), ("gt", gt, False, "gt" in kinds and has_gt)]
        return [(name,) + hw + (rnd,) for name, hw, rnd, on in use if on]

    def open(self, ms, rec, L, **room):
        has_gt = "sse" in rec                              # without ground truth, lr and esr only
        if max(h * w for h, w in (self.size(ms, k, has_gt) for k in ms.render)) > slots.MAX_RENDER_PIXELS:
            raise ValueError("MultiStreamSR: images of more than 2^24 pixels cannot be rendered (sizes %s)" % (ms._size,))
        rec["images"] = {k: torch.empty((rec["n"],) + self.size(ms, k, has_gt) + (3,), dtype=U8, device=rec["device"])
                         for k in ms.render if has_gt or k in ("lr", "esr")}

    def scratch(self, ms):
        names = [t[0] for t in self.tables(ms)]
        d = {"render_minmax": ((4 * ms.S,), F32, 0, True)}
        if "esr_gt" in names or "bicubic" in names:
            d["render_resize"] = ((ms.S, 2) + tuple(ms._size[2:]), F32, 0, True)
        if "bicubic" in names:
            d["render_mid"] = ((ms.S, 2) + tuple(ms._size[:2]), F32, 0, True)
        if "esr" in names and ms.self_ensemble:            # the merged predictions, at an address the table can name
            d["render_pred"] = ((ms.S, 2, ms.scale * ms._size[0], ms.scale * ms._size[1]), F32, 0, True)
        return d

    def fill(self, ms, v, s, r, i, reset):
        """Where each of the recording's pictures reads its count image; the slot entry has been filled."""
        e, rn = v["slot"][s], v["render"]
        b, (H, W) = ms._bufs, ms._size[:2]
        resized = "sse" in r and tuple(ms._size[2:]) != (ms.scale * H, ms.scale * W)
        for kind, img in r["images"].items():
            if kind == "lr":                               # frame 1 of the window
                table, src = "lr", int(e["frames"]) + 4 * 2 * H * W
            elif kind == "esr":
                table, src = ("esr_gt", b["render_resize"][s].data_ptr()) if resized else \
                    ("esr", b["render_pred" if ms.self_ensemble else "pred"][s].data_ptr())
            elif kind == "bicubic":
                table, src = "bicubic", b["render_resize"][s].data_ptr()
            else:
                table, src = "gt", int(e["gt"])
            k = self.TABLES.index(table)
            rn[k, s]["src"], rn[k, s]["dst"] = src, img[i].data_ptr()

    def launch(self, ms, b, pred):
        # "esr" reads b["pred"], where commit has put the predictions; the resize scratch serves the prediction first, then frame 1.
        # A self-ensemble session: b["pred"] holds every member's OWN prediction (its recurrence), the merged one is in the leader's
        # row of `pred`, the model's output, which has no lasting address: "esr" reads a copy of it
        S, (H, W) = ms.S, ms._size[:2]
        for name, h, w, rnd in self.tables(ms):
            if name == "esr" and ms.self_ensemble:
                b["render_pred"].copy_(pred)
            elif name == "esr_gt":
                lib.call(lib._bicubic_fwd, "bmc_bicubic_resize_fwd", pred.data_ptr(), 2 * S, ms.scale * H, ms.scale * W, h, w,
                         b["render_resize"].data_ptr(), _stream())
            elif name == "bicubic":
                b["render_mid"].copy_(b["x"][:, :, 1])     # frame 1 of every slot's window, as stage gathered it: [S,2,H,W]
                lib.call(lib._bicubic_fwd, "bmc_bicubic_resize_fwd", b["render_mid"].data_ptr(), 2 * S, H, W, h, w,
                         b["render_resize"].data_ptr(), _stream())
            slots.render(b["table"], self.TABLES.index(name), h, w, rnd, b["render_minmax"])

    def results(self, ms, out, r, done, handle):
        out["images"] = {k: t[:done] for k, t in r["images"].items()}


class VoxelGrids(Part):
    """voxel_bins=B (1 <= B <= 32; needs max_count <= 255): every window's prediction also leaves as the temporal-bilinear VOXEL
    GRID of its super-resolved events, the input form of reconstruction, flow and recognition networks: what the reference's
    events_to_voxel_torch (dataloader/encodings.py:100-148) returns for the window's timed event stream (the stream of
    event_times="linear"), bit for bit, computed per output pixel from the prediction's two counts and one small reduction
    (bmc_slot_voxel: two more launches per window for all slots, inside the captured graph too; no sort, no atomics, no event
    storage; include/bmc_hip.h "voxel grids" states the contract).  Independent of emit_events, event_times and render, for
    frame-backed and event-backed recordings, with or without ground truth.  results() then carries voxels = float32
    [done,B,sH,sW] on the GPU, at the prediction's own size; its rows are the sensor's y, vertically flipped against the
    prediction's rows as the emitted ys are.  The grid is window-normalised, so a sensor clock does not change it.  Resident:
    4 x B x sH x sW bytes per window -- 13.8 MB per window at 720x960 with 5 bins; session scratch: the partials of the reduce
    launch (8 bytes per part and slot)."""

    @staticmethod
    def check(voxel_bins, max_count):
        if voxel_bins is None:
            return None
        if isinstance(voxel_bins, bool) or not isinstance(voxel_bins, (int, np.integer)) or not 1 <= voxel_bins <= slots.MAX_VOXEL_BINS:
            raise ValueError("MultiStreamSR: voxel_bins must be None or an integer, 1 <= voxel_bins <= %d (got %r)"
                             % (slots.MAX_VOXEL_BINS, voxel_bins))
        if max_count > slots.MAX_COUNT_TIMED:
            raise ValueError("MultiStreamSR: voxel_bins needs max_count <= %d (the timed stream's limit; got %d)"
                             % (slots.MAX_COUNT_TIMED, max_count))
        return int(voxel_bins)

    def table(self, ms):
        return {"voxel": True}

    def open(self, ms, rec, L, **room):
        sH, sW = ms.scale * ms._size[0], ms.scale * ms._size[1]
        if max(sH, sW) > slots.MAX_COUNT_LIMIT:
            raise ValueError("MultiStreamSR: predictions of %d x %d are too large for voxel grids (at most %d a side)"
                             % (sH, sW, slots.MAX_COUNT_LIMIT))
        rec["voxels"] = torch.empty(rec["n"], ms.voxel_bins, sH, sW, device=rec["device"])

    def scratch(self, ms):
        return {"voxel_parts": ((2 * ms.S * ms._vparts,), I32, 0, True)}

    def fill(self, ms, v, s, r, i, reset):
        v["voxel"][s]["dst"] = r["voxels"][i].data_ptr()

    def launch(self, ms, b, pred):
        slots.voxel(b["table"], pred, ms.max_count, ms.voxel_bins, ms._vparts, b["voxel_parts"])

    def results(self, ms, out, r, done, handle):
        out["voxels"] = r["voxels"][:done]
