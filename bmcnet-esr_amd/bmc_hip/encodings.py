"""GPU event encodings with the reference's function signature
(reference: dataloader/encodings.py:290-305 events_to_channels, :241-269 events_to_image).

The scatter runs on the MI355X (bmc_events_to_channels, one float atomic per event, bit-exact with the
reference including its out-of-range quirk and its in-place reset of the caller's xs/ys).  CPU tensors
are rejected: there is no CPU fallback."""
import math

import numpy as np
import torch

from . import lib, ops


def events_to_channels(xs, ys, ps, sensor_size=(180, 240)):
    """Two-channel event count image [2,H,W] from fp32 event vectors on the GPU.
    As in the reference, out-of-range entries of the caller's xs/ys are reset to 0 in place."""
    assert len(xs) == len(ys) and len(ys) == len(ps)
    if not (xs.is_cuda and ys.is_cuda and ps.is_cuda):
        raise RuntimeError("events_to_channels: tensors must live on the MI355X (no CPU fallback in this build)")
    if not (xs.is_contiguous() and ys.is_contiguous() and ps.is_contiguous()):
        raise RuntimeError("events_to_channels: xs/ys/ps must be contiguous (they are updated in place)")
    off = torch.tensor([0, xs.numel()], dtype=torch.int64, device=xs.device)
    return ops.events_to_channels_batched(xs, ys, ps, off, int(sensor_size[0]), int(sensor_size[1]), mutate=True)[0]


def events_to_voxel(xs, ys, ts, ps, num_bins, sensor_size=(180, 240)):
    """Voxel grid [num_bins,H,W] with temporal bilinear interpolation (reference: dataloader/encodings.py:272-287),
    on GPU tensors; as in the reference the caller's xs/ys lose their out-of-range entries (reset to 0)."""
    assert len(xs) == len(ys) and len(ys) == len(ts) and len(ts) == len(ps)
    if not (xs.is_cuda and ys.is_cuda and ts.is_cuda and ps.is_cuda):
        raise RuntimeError("events_to_voxel: tensors must live on the MI355X (no CPU fallback in this build)")
    off = torch.tensor([0, xs.numel()], dtype=torch.int64, device=xs.device)
    return ops.events_to_voxel_batched(xs, ys, ts, ps, off, int(num_bins), int(sensor_size[0]), int(sensor_size[1]))[0]


def events_to_stack_no_polarity(xs, ys, ts, ps, B, device=None, sensor_size=(180, 240)):
    """Event stack [B,H,W]: B temporal bins, each the signed per-pixel sum of its events' polarities (reference:
    dataloader/encodings.py:202-238, same signature).  On GPU tensors; like the reference it returns zeros for windows
    of <= 3 events or all-zero timestamps, and zeroes the out-of-range events of the caller's xs / ys / ps in place."""
    assert len(xs) == len(ys) and len(ys) == len(ts) and len(ts) == len(ps)
    if not (xs.is_cuda and ys.is_cuda and ts.is_cuda and ps.is_cuda):
        raise RuntimeError("events_to_stack_no_polarity: tensors must live on the MI355X (no CPU fallback in this build)")
    H, W = int(sensor_size[0]), int(sensor_size[1])
    if len(ts) <= 3 or ts.sum() == 0:
        return torch.zeros([B, H, W], device=xs.device)
    return ops.events_to_stack(xs, ys, ts, ps, int(B), H, W)


def events_to_stack_polarity(xs, ys, ts, ps, B, device=None, sensor_size=(180, 240)):
    """Polarity-split event stack [2,B,H,W] (reference: dataloader/encodings.py:151-199, same signature) on GPU tensors;
    like the reference: [B,H,W] zeros for windows of <= 3 events or all-zero timestamps, and the caller's xs / ys lose their
    out-of-range entries (ps is left alone)."""
    assert len(xs) == len(ys) and len(ys) == len(ts) and len(ts) == len(ps)
    if not (xs.is_cuda and ys.is_cuda and ts.is_cuda and ps.is_cuda):
        raise RuntimeError("events_to_stack_polarity: tensors must live on the MI355X (no CPU fallback in this build)")
    H, W = int(sensor_size[0]), int(sensor_size[1])
    if ts.sum() == 0 or len(ts) <= 3:
        return torch.zeros([B, H, W], device=xs.device)
    return ops.events_to_stack_polarity(xs, ys, ts, ps, int(B), H, W)


def events_to_mask(xs, ys, ps, sensor_size=(180, 240)):
    """Binary event mask [H,W] (reference: dataloader/encodings.py:308-332, same signature) on GPU tensors; as in the
    reference the caller's xs / ys / ps lose their out-of-range entries in place."""
    if not (xs.is_cuda and ys.is_cuda and ps.is_cuda):
        raise RuntimeError("events_to_mask: tensors must live on the MI355X (no CPU fallback in this build)")
    if not (xs.is_contiguous() and ys.is_contiguous() and ps.is_contiguous()):
        raise RuntimeError("events_to_mask: xs/ys/ps must be contiguous (they are updated in place)")
    return ops.events_to_mask(xs, ys, ps, int(sensor_size[0]), int(sensor_size[1]))


def get_hot_event_mask(event_rate, idx, max_px=100, min_obvs=5, max_rate=0.8):
    """Binary mask [H,W] (1 = keep) that removes the events of hot pixels (reference: dataloader/encodings.py:349-364, same
    signature) on a contiguous float32 GPU tensor: if idx > min_obvs, the entries > max_rate, at most max_px of them, the
    largest first and equal ones in flat order; as in the reference the selected entries of event_rate are zeroed in place.
    bmc_hot_pixel_mask (include/bmc_hip.h) states the special values: any NaN masks nothing, -0.0 orders as +0.0, and a
    negative max_rate spends what max_px leaves on one more entry."""
    if not (torch.is_tensor(event_rate) and event_rate.is_cuda):
        raise RuntimeError("get_hot_event_mask: event_rate must live on the MI355X (no CPU fallback in this build)")
    if not (event_rate.dim() == 2 and event_rate.dtype == torch.float32 and event_rate.is_contiguous() and event_rate.numel()):
        raise RuntimeError("get_hot_event_mask: event_rate must be a contiguous float32 [H,W] tensor (it is updated in place)")
    H, W = event_rate.shape
    mask = torch.empty_like(event_rate)
    ws = torch.empty(H * W, dtype=torch.int32, device=event_rate.device)
    lib.call(lib._hot_pixel_mask, "bmc_hot_pixel_mask", event_rate.data_ptr(), H, W, int(idx > min_obvs),
             max(0, min(int(max_px), H * W)), float(max_rate), mask.data_ptr(), ws.data_ptr(), ops._stream())
    return mask


def _noise_columns(who, xs, ys, ts, ps):
    """The column checks of the noise filter that need no device round trip: types, shapes, lengths, one GPU."""
    cols = [("xs", xs, torch.int16), ("ys", ys, torch.int16), ("ts", ts, torch.float64)] + ([] if ps is None else [("ps", ps, torch.float64)])
    for name, t, dtype in cols:
        if not (torch.is_tensor(t) and t.dtype == dtype and t.dim() == 1 and t.is_contiguous()):
            raise ValueError(who + "%s must be a contiguous 1-D %s tensor" % (name, str(dtype).replace("torch.", "")))
        if t.numel() != xs.numel():
            raise ValueError(who + "%s has %d entries, xs %d" % (name, t.numel(), xs.numel()))
    if not all(t.is_cuda and t.device == xs.device for _, t, _ in cols):
        raise ValueError(who + "the columns must be GPU tensors on one device (no CPU fallback in this build)")
    if xs.numel() >= 1 << 31:
        raise ValueError(who + "streams of 2^31 events or more are not supported")


def _noise_size(who, sensor_size):
    from . import denoise_lib
    try:
        H, W = (int(v) for v in sensor_size)
    except (TypeError, ValueError):
        raise ValueError(who + "sensor_size = (H, W)") from None
    if H < 1 or W < 1 or W > denoise_lib.MAX_W:
        raise ValueError(who + "sensor_size must be positive and at most %d wide (got %s)" % (denoise_lib.MAX_W, (H, W)))
    return H, W


def _noise_numbers(who, dt, support, names=("dt", "support")):
    from . import denoise_lib
    if isinstance(dt, bool) or not isinstance(dt, (int, float, np.integer, np.floating)) or not math.isfinite(dt) or dt < 0:
        raise ValueError(who + "%s must be a finite number >= 0, in the units of ts (got %r)" % (names[0], dt))
    if isinstance(support, bool) or not isinstance(support, (int, np.integer)) or not 1 <= support <= denoise_lib.MAX_SUPPORT:
        raise ValueError(who + "%s must be an integer, 1 <= support <= %d (got %r)" % (names[1], denoise_lib.MAX_SUPPORT, support))
    return float(dt), int(support)


NOISE_CALLS = 0     # calls of bmc_event_denoise so far (tests: one per filtered recording at the door, none per window)


def _event_noise(xs, ys, ts, H, W, dt, support, ps=None, keep=True, count=False):
    """bmc_event_denoise on checked columns, on the current stream, no sync -> (keep or None, ps_out or None, kept or None),
    kept a 1-element int64 GPU tensor."""
    global NOISE_CALLS
    from . import denoise_lib
    NOISE_CALLS += 1
    n, dev = xs.numel(), xs.device
    keep = torch.empty(n, dtype=torch.uint8, device=dev) if keep else None
    ps_out = None if ps is None else torch.empty_like(ps)
    kept = torch.empty(1, dtype=torch.int64, device=dev) if count else None
    scratch = torch.empty(denoise_lib.scratch_bytes(H, W) // 8, dtype=torch.int64, device=dev) if count else None
    ptr = lambda t: None if t is None else t.data_ptr()
    lib.call(denoise_lib._event_denoise, "bmc_event_denoise", xs.data_ptr(), ys.data_ptr(), ts.data_ptr(), ptr(ps), n, H, W, dt,
             support, ptr(keep), ptr(ps_out), ptr(kept), ptr(scratch), ops._stream())
    return keep, ps_out, kept


def event_noise_mask(xs, ys, ts, sensor_size, dt, support=1, ps=None):
    """The background-activity (nearest-neighbour correlation) filter of one raw event stream, on the GPU (the contract:
    include/bmc_hip_denoise.h): keep[i] = 1 iff event i is inside the sensor and at least `support` of the eight pixels around
    it saw their latest earlier event no more than dt before it.  support = 1 is jAER's BackgroundActivityFilter, support > 1
    its SpatioTemporalCorrelationFilter.  xs, ys int16, ts float64 (finite and non-decreasing: NOT checked here -- the check
    would wait for the device; check_noise_filter does it), in column order, 1-D contiguous GPU tensors.
    -> keep (uint8) or, with ps (float64), (keep, ps_out): ps with the dropped events' polarities replaced by +0.0, which every
    encoder of the library counts as nothing.  One call of bmc_event_denoise on the current stream; nothing waits for it."""
    who = "event_noise_mask: "
    _noise_columns(who, xs, ys, ts, ps)
    H, W = _noise_size(who, sensor_size)
    dt, support = _noise_numbers(who, dt, support)
    keep, ps_out, _ = _event_noise(xs, ys, ts, H, W, dt, support, ps)
    return keep if ps is None else (keep, ps_out)


def check_noise_filter(who, noise_filter, columns=None, sensor_size=None):
    """noise_filter (None, or a dict with exactly the keys ts, dt and, optionally, support) -> None or (ts, dt, support), the
    arguments of event_noise_mask; ValueError names the bad key, as slots.check_hot_filter.  ts: the stream's float64 timestamp
    column, finite and non-decreasing (one reduction on its device); dt: finite, >= 0; support: an integer 1 .. 8 (default 1).
    columns = (xs, ys, ps) and sensor_size = (H, W) of the stream the filter is for: their types and lengths, ts parallel to
    them on the same GPU, and the width within the kernel's limit."""
    if noise_filter is None:
        return None
    keys = ("ts", "dt", "support")
    if not isinstance(noise_filter, dict):
        raise ValueError(who + "noise_filter must be None or a dict with the keys %s (got %r)" % (", ".join(keys), noise_filter))
    for k in noise_filter:
        if k not in keys:
            raise ValueError(who + "noise_filter has an unknown key %r (the keys are %s)" % (k, ", ".join(keys)))
    for k in keys[:2]:
        if k not in noise_filter:
            raise ValueError(who + "noise_filter lacks the key %r" % k)
    ts = noise_filter["ts"]
    dt, support = _noise_numbers(who, noise_filter["dt"], noise_filter.get("support", 1), ("noise_filter['dt']", "noise_filter['support']"))
    if not (torch.is_tensor(ts) and ts.dtype == torch.float64 and ts.dim() == 1 and ts.is_contiguous()):
        raise ValueError(who + "noise_filter['ts'] must be a contiguous 1-D float64 tensor")
    if columns is not None:
        xs, ys, ps = columns
        _noise_columns(who + "noise_filter: ", xs, ys, ts, ps)
    if sensor_size is not None:
        _noise_size(who + "noise_filter: ", sensor_size)
    if ts.numel() and not bool(torch.isfinite(ts).all() & (ts[1:] >= ts[:-1]).all()):
        raise ValueError(who + "noise_filter['ts'] must be finite and non-decreasing")
    return ts, dt, support


def filter_noise(who, noise_filter, columns, sensor_size):
    """(xs, ys, ps) of a recording through its noise_filter -> ((xs, ys, ps_out), events dropped); the caller's ps is not
    modified.  What open_events(noise_filter=...) and EventTrainSet.add_recording(noise_filter=...) do at the door."""
    ts, dt, support = check_noise_filter(who, noise_filter, columns, sensor_size)
    xs, ys, ps = columns
    _, ps_out, kept = _event_noise(xs, ys, ts, int(sensor_size[0]), int(sensor_size[1]), dt, support, ps, keep=False, count=True)
    return (xs, ys, ps_out), xs.numel() - int(kept.item())


DOWNSAMPLE_CALLS = 0    # streams downsampled so far (tests: one per HR-only recording at the door, none per window or batch)
DOWNSAMPLE_LAUNCHES = 0  # launches of the library those calls made (downsample_lib.LAUNCHES each; 2 for an empty stream)


def downsample_geometry(who, sensor_size, scale, threshold=None):
    """The number checks of downsample_events -> (H, W, s, T, (h, w)): sensor_size = (H, W) positive; scale an integer 1 .. 16;
    threshold an integer 1 .. 32767, None = scale^2; (h, w) = the LR sensor, ceil(H / s) x ceil(W / s)."""
    from . import downsample_lib
    try:
        H, W = (int(v) for v in sensor_size)
    except (TypeError, ValueError):
        raise ValueError(who + "sensor_size = (H, W)") from None
    if H < 1 or W < 1:
        raise ValueError(who + "sensor_size must be positive (got %s)" % ((H, W),))
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or not 1 <= scale <= downsample_lib.MAX_SCALE:
        raise ValueError(who + "scale must be an integer, 1 <= scale <= %d (got %r)" % (downsample_lib.MAX_SCALE, scale))
    s = int(scale)
    T = s * s if threshold is None else threshold
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or not 1 <= T <= downsample_lib.MAX_THRESHOLD:
        raise ValueError(who + "threshold must be an integer, 1 <= threshold <= %d, or None for scale^2 (got %r)"
                         % (downsample_lib.MAX_THRESHOLD, threshold))
    h, w = -(-H // s), -(-W // s)
    if h * w >= (1 << 31) - 1:
        raise ValueError(who + "%d x %d LR pixels are not below 2^31 - 1" % (h, w))
    return H, W, s, int(T), (h, w)


def check_downsample(who, xs, ys, ts, ps, sensor_size, scale, threshold=None):
    """The checks of downsample_events, none of which waits for the device -> downsample_geometry's tuple: the numbers, then
    column types, shapes, lengths, one GPU (as check_noise_filter's columns)."""
    geometry = downsample_geometry(who, sensor_size, scale, threshold)
    if ps is None:
        raise ValueError(who + "ps must be a contiguous 1-D float64 tensor")
    _noise_columns(who, xs, ys, ts, ps)
    return geometry


def _event_downsample(xs, ys, ts, ps, H, W, s, T):
    """The four stages of include/bmc_hip_downsample.h on checked columns, on the current stream, no sync -> (xs, ys, ts, ps,
    count): output columns of capacity n // T and a 1-element int64 GPU tensor."""
    global DOWNSAMPLE_CALLS, DOWNSAMPLE_LAUNCHES
    from . import downsample_lib as D
    DOWNSAMPLE_CALLS += 1
    n, dev, stream = xs.numel(), xs.device, ops._stream()
    cap = D.capacity(n, T)
    out = (torch.empty(cap, dtype=torch.int16, device=dev), torch.empty(cap, dtype=torch.int16, device=dev),
           torch.empty(cap, dtype=torch.float64, device=dev), torch.empty(cap, dtype=torch.float64, device=dev))
    count = torch.empty(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(D.scratch_bytes(n) // 8, dtype=torch.int64, device=dev)
    fire = torch.empty(n, dtype=torch.int8, device=dev)
    if n:
        keys = torch.empty(n, dtype=torch.int32, device=dev)
        lib.call(D._keys, "bmc_event_downsample_keys", xs.data_ptr(), ys.data_ptr(), ps.data_ptr(), n, H, W, s, keys.data_ptr(),
                 fire.data_ptr(), stream)
        keys, perm = torch.sort(keys, stable=True)                   # the grouping: every LR pixel's events, in column order
        lib.call(D._walk, "bmc_event_downsample_walk", keys.data_ptr(), perm.data_ptr(), ps.data_ptr(), n, H, W, s, T,
                 fire.data_ptr(), stream)
        DOWNSAMPLE_LAUNCHES += 2
    ptr = lambda t: t.data_ptr() if t.numel() else None
    lib.call(D._gather, "bmc_event_downsample_gather", ptr(xs), ptr(ys), ptr(ts), ptr(fire), n, s, *(ptr(t) for t in out), cap,
             count.data_ptr(), scratch.data_ptr(), stream)
    DOWNSAMPLE_LAUNCHES += 2
    return out + (count,)


def downsample_events(xs, ys, ts, ps, sensor_size, scale, threshold=None, trim=True):
    """The LR event stream of an HR stream by integrate-and-fire over blocks of scale x scale pixels, on the GPU (the contract:
    include/bmc_hip_downsample.h): an LR pixel adds the +1 / -1 steps of the counted events of its block in column order and
    fires, and starts again from 0, when the sum reaches +threshold or -threshold (None: scale^2, one LR contrast step of the
    block's mean).  An event with polarity +-0.0 or NaN, or outside the sensor, touches nothing.
    xs, ys int16, ts float64 (non-decreasing: the caller's business; the result depends on column order only), ps float64, 1-D
    contiguous GPU tensors; sensor_size = (H, W) of the HR sensor.  The caller's tensors are not modified.
    -> (xs, ys, ts, ps, lr_size): int16, int16, float64 (the firing events' own timestamps), float64 (+-1.0) GPU tensors --
    the column types open_events / add_recording take -- and lr_size = (ceil(H / scale), ceil(W / scale)).
    trim=True cuts the columns to the number of LR events, which costs ONE host sync, the only one.  trim=False waits for
    nothing: -> (xs, ys, ts, ps, lr_size, count), the columns at their capacity n // threshold, count a 1-element int64 GPU
    tensor, entries at count and after unwritten.  One stable torch.sort of n int32 keys plus downsample_lib.LAUNCHES launches."""
    who = "downsample_events: "
    H, W, s, T, lr_size = check_downsample(who, xs, ys, ts, ps, sensor_size, scale, threshold)
    oxs, oys, ots, ops_, count = _event_downsample(xs, ys, ts, ps, H, W, s, T)
    if not trim:
        return oxs, oys, ots, ops_, lr_size, count
    k = int(count.item())
    return oxs[:k], oys[:k], ots[:k], ops_[:k], lr_size


def check_hr_noise_filter(who, noise_filter):
    """noise_filter of an HR-only recording (None, or a dict with the keys dt and, optionally, support: ts is the synthesized
    column, which the caller cannot have) -> None or dict(dt=, support=), checked as check_noise_filter checks them."""
    if noise_filter is None:
        return None
    if not isinstance(noise_filter, dict) or "dt" not in noise_filter or set(noise_filter) - {"dt", "support"}:
        raise ValueError(who + "noise_filter must be None or a dict with the keys dt, support (ts is the synthesized column; got %r)"
                         % (noise_filter,))
    dt, support = _noise_numbers(who, noise_filter["dt"], noise_filter.get("support", 1), ("noise_filter['dt']", "noise_filter['support']"))
    return dict(dt=dt, support=support)


def synthesize_lr(who, gt, gt_ts, gt_size, scale, threshold=None):
    """(xs, ys, ps) and the timestamp column of an HR-only recording -> ((xs, ys, ps), lr_ts, lr_size) of its synthetic LR stream
    (downsample_events, trimmed: one host sync).  What EventTrainSet.add_hr_recording and MultiStreamSR.open_hr_events do at the
    door."""
    if not (isinstance(gt, (tuple, list)) and len(gt) == 3 and all(torch.is_tensor(t) for t in gt)):
        raise ValueError(who + "gt must be three tensors (xs, ys, ps)")
    if not torch.is_tensor(gt_ts):
        raise ValueError(who + "gt_ts must be a contiguous 1-D float64 tensor")
    H, W, s, T, lr_size = check_downsample(who, gt[0], gt[1], gt_ts, gt[2], gt_size, scale, threshold)
    xs, ys, ts, ps, count = _event_downsample(gt[0], gt[1], gt_ts, gt[2], H, W, s, T)
    k = int(count.item())
    return (xs[:k], ys[:k], ps[:k]), ts[:k], lr_size


def events_to_channels_batch(xs, ys, ps, offsets, sensor_size=(180, 240), mutate=True):
    """Many frames in one launch: frame f owns events [offsets[f], offsets[f+1]) -> [nframes,2,H,W]."""
    return ops.events_to_channels_batched(xs, ys, ps, offsets, int(sensor_size[0]), int(sensor_size[1]), mutate=mutate)


def augment_flags(seed, mechanisms=("Horizontal", "Vertical", "Polarity"), probs=(0.5, 0.5, 0.5)):
    """Flip decisions of H5Dataset.augment_event (dataloader/h5dataset.py:559-578) for one sample seed, as the bit
    flags bmc_encode_raw_events takes (bit0 horizontal, bit1 vertical, bit2 polarity).  Same seeding as the reference:
    random.seed(seed), seed+1, seed+2 for H / V / P, one random.random() draw each; the caller's `random` state is
    left as the reference leaves it (re-seeded).  "Transpose" (not the reference's; bit3, which only bmc_seq_encode_crop
    reads) follows the pattern: random.seed(seed+3), one draw.  Other names are skipped."""
    import random
    flags = 0
    for i, mech in enumerate(mechanisms):
        if mech == "Horizontal":
            random.seed(seed)
            if random.random() < probs[i]:
                flags |= 1
        elif mech == "Vertical":
            random.seed(seed + 1)
            if random.random() < probs[i]:
                flags |= 2
        elif mech == "Polarity":
            random.seed(seed + 2)
            if random.random() < probs[i]:
                flags |= 4
        elif mech == "Transpose":
            random.seed(seed + 3)
            if random.random() < probs[i]:
                flags |= 8
    return flags


def raw_events_to_channels_batch(xs_i16, ys_i16, ps_f64, offsets, flips=None, sensor_size=(180, 240)):
    """GPU sequence encoder on raw HDF5 columns (int16 x/y, float64 p) with the flip augmentation folded in:
    replaces get_events -> augment_event -> event_formatting -> events_to_channels of the CPU workers."""
    return ops.encode_raw_events(xs_i16, ys_i16, ps_f64, offsets, flips, int(sensor_size[0]), int(sensor_size[1]))


def event_window_indices(lr_ts, gt_ts, window=2048, sliding_window=1024, scale=4, dataset_length=None, mode="events"):
    """The event blocks H5Dataset cuts a recording into for mode == 'events' (dataloader/h5dataset.py: set_data_mode
    :164-195, compute_k_indices :197-215, get_gt_event_indices_num :362-390), from the two timestamp columns alone (numpy, on
    the CPU) -> (lr_index [L,2], gt_index [L,2]) int64: item j is LR events [lr_index[j,0], lr_index[j,1]) and HR events
    [gt_index[j,0], gt_index[j,1]) (what get_events / get_gt_events slice, :407-424).  The reference's quirks are kept:
      * L = int(num_events / (window - sliding_window)), capped by dataset_length; L == 0 raises as the reference does;
      * idx1 = idx0 + window clamped to num_events - 1: the tail blocks are shorter and the last LR event is never used;
      * every HR block has scale^2 * (idx1 - idx0) events OF BLOCK 0, also where the LR block itself is shorter;
      * the HR block starts at the first HR event with ts >= the LR block's first ts, found by ONE forward scan that hands
        out each HR event at most once (base_dataset.py:39-51): a block whose start the previous block already took starts
        one event later;
      * an HR block that would end after num_gt_events - 1 is moved back to end there (which can push its start below zero:
        the reference then fails in get_gt_event_indices; MultiStreamSR.open_events refuses such a table);
      * LR blocks that start after the last HR timestamp get no HR block in the reference (its item access fails there):
        both tables end at the last block that has one.
    gt_ts=None: a recording WITHOUT ground truth (need_gt_events=False, h5dataset.py:278-279) -> (lr_index, None): the blocks
    compute_k_indices cuts (the first two rules above) with no truncation by HR coverage.  For a stream that has a ground
    truth this is the table returned with it, possibly followed by further rows.
    Only 'events' mode: the reference's 'time' and 'frame' modes call get_gt_event_indices_num(start_idx, end_idx) with two
    arguments where it takes one (:231, :245) and cannot run with ground-truth events -> ValueError."""
    import numpy as np
    if mode != "events":
        raise ValueError("event_window_indices: only mode='events' (the reference's %r mode cannot run with ground-truth "
                         "events)" % (mode,))
    lr_ts = np.asarray(lr_ts)
    gt_ts = None if gt_ts is None else np.asarray(gt_ts)
    if lr_ts.ndim != 1 or (gt_ts is not None and gt_ts.ndim != 1):
        raise ValueError("event_window_indices: lr_ts and gt_ts are 1-D timestamp columns")
    step = int(window) - int(sliding_window)
    if step <= 0:
        raise ValueError("event_window_indices: window must exceed sliding_window")
    n = len(lr_ts)
    L = max(int(n / step), 0)
    if dataset_length is not None:
        L = min(int(dataset_length), L)
    if L <= 0:
        raise ValueError("event_window_indices: %d events give no block of %d advancing by %d" % (n, window, step))
    idx0 = step * np.arange(L, dtype=np.int64)
    idx1 = np.minimum(idx0 + int(window), n - 1)
    if gt_ts is None:
        return np.stack([idx0, idx1], 1), None
    n_gt = len(gt_ts)
    num_gt = int(scale) ** 2 * int(idx1[0] - idx0[0])
    first = np.searchsorted(gt_ts, lr_ts[idx0], side="left").astype(np.int64)
    k = np.arange(L, dtype=np.int64)
    g0 = np.maximum.accumulate(first - k) + k              # each HR event is handed out once: g0[j] >= g0[j-1] + 1
    keep = int(np.count_nonzero(g0 < n_gt))
    idx0, idx1, g0 = idx0[:keep], idx1[:keep], g0[:keep]
    g1 = g0 + num_gt
    over = g1 > n_gt - 1
    g1 = np.where(over, n_gt - 1, g1)
    g0 = np.where(over, g1 - num_gt, g0)
    return np.stack([idx0, idx1], 1), np.stack([g0, g1], 1)


def event_block_spans(lr_ts, lr_index):
    """The time span of every item of a recording on its own clock -> [L,2] float64 on the host: for item j = events
    [first, end) of lr_index, (t_first, t_last) = (lr_ts[first], lr_ts[end - 1]); an empty item gets lr_ts[min(first, n - 1)]
    twice.  lr_ts: the recording's timestamp column (1-D, n >= 1 entries; a numpy array or a tensor on the host or the GPU --
    there one gather and one copy); lr_index: an integer [L,2] table with 0 <= first <= end <= n.  What
    MultiStreamSR.open_events(lr_ts=...) hands to the clocked event output."""
    import numpy as np
    idx = np.asarray(lr_index.cpu() if torch.is_tensor(lr_index) else lr_index)
    if idx.ndim != 2 or idx.shape[1] != 2 or idx.dtype.kind not in "iu":
        raise ValueError("event_block_spans: lr_index must be an integer [L,2] table (got %s %s)" % (idx.dtype, idx.shape))
    idx = idx.astype(np.int64)
    n = lr_ts.numel() if torch.is_tensor(lr_ts) else np.asarray(lr_ts).size
    if (lr_ts.dim() if torch.is_tensor(lr_ts) else np.asarray(lr_ts).ndim) != 1 or n < 1:
        raise ValueError("event_block_spans: lr_ts is a 1-D timestamp column of at least one event")
    if (idx[:, 0] > idx[:, 1]).any() or (idx.size and (idx.min() < 0 or idx.max() > n)):
        raise ValueError("event_block_spans: lr_index has a range outside the %d events of the column" % n)
    empty = idx[:, 0] == idx[:, 1]
    first = np.where(empty, np.minimum(idx[:, 0], n - 1), idx[:, 0])
    last = np.where(empty, first, idx[:, 1] - 1)
    take = np.stack([first, last], 1).reshape(-1)
    if torch.is_tensor(lr_ts):
        got = lr_ts.index_select(0, torch.from_numpy(take).to(lr_ts.device)).to("cpu", torch.float64).numpy()
    else:
        got = np.asarray(lr_ts)[take].astype(np.float64)
    return got.reshape(-1, 2)


def check_spans(who, spans, L):
    """spans -> a [L,2] float64 numpy table of finite (t_first, t_last) with t_last >= t_first, or ValueError."""
    import numpy as np
    a = np.asarray(spans.cpu() if torch.is_tensor(spans) else spans)
    if a.ndim != 2 or a.shape != (L, 2) or a.dtype.kind not in "fiu":
        raise ValueError(who + "spans must be a [%d,2] table of (t_first, t_last) (got %s %s)" % (L, a.dtype, a.shape))
    a = a.astype(np.float64)
    if not np.isfinite(a).all() or (a[:, 1] < a[:, 0]).any():
        raise ValueError(who + "every span must be finite with t_last >= t_first")
    return a


def events_to_image_torch(xs, ys, ps, device=None, sensor_size=(180, 240), clip_out_of_range=True, interpolation=None, padding=True):
    """events_to_image_torch of the reference (dataloader/encodings.py:16-73) on the GPU: same signature, same side effects
    (out-of-range events are reset in place to (0, 0) with weight 0), same summation order as its CPU index_put_ -> bit-identical.
    xs / ys / ps: contiguous float32 CUDA tensors (sub-pixel positions for interpolation='bilinear')."""
    import ctypes as C
    from . import lib, ops
    if interpolation not in (None, "bilinear"):
        raise ValueError("interpolation must be None or 'bilinear'")
    for t in (xs, ys, ps):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("bmc_hip.encodings.events_to_image_torch needs contiguous float32 CUDA tensors (the reference's long-"
                               "coordinate variant: convert with .float())")
    H, W = sensor_size
    bil = interpolation == "bilinear"
    shape = (H + 1, W + 1) if (bil and padding) else (H, W)
    n = xs.numel()
    out = torch.empty(shape, device=xs.device, dtype=torch.float32)
    ws = torch.empty(lib._ev_torch_ws(n, H, W), device=xs.device, dtype=torch.int32)
    lib.call(lib._ev_img_torch, "bmc_events_to_image_torch", xs.data_ptr(), ys.data_ptr(), ps.data_ptr(), n, H, W,
             1 if clip_out_of_range else 0, 1 if bil else 0, 1 if padding else 0, out.data_ptr(), ws.data_ptr(), ops._stream())
    return out


def events_to_voxel_torch(xs, ys, ts, ps, B, device=None, sensor_size=(180, 240), temporal_bilinear=True):
    """events_to_voxel_torch of the reference (dataloader/encodings.py:100-148), temporal_bilinear=True, on the GPU: [B, H, W];
    zeros for <= 3 events or all-zero timestamps; xs / ys are reset in place where out of range, as the reference does."""
    from . import lib, ops
    if not temporal_bilinear:
        raise NotImplementedError("bmc_hip.encodings.events_to_voxel_torch: only temporal_bilinear=True is implemented")
    for t in (xs, ys, ts, ps):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("bmc_hip.encodings.events_to_voxel_torch needs contiguous float32 CUDA tensors")
    H, W = sensor_size
    n = xs.numel()
    out = torch.empty((B, H, W), device=xs.device, dtype=torch.float32)
    ws = torch.empty(lib._ev_torch_ws(n, H, W), device=xs.device, dtype=torch.int32)
    lib.call(lib._ev_vox_torch, "bmc_events_to_voxel_torch", xs.data_ptr(), ys.data_ptr(), ts.data_ptr(), ps.data_ptr(), n, B, H, W,
             out.data_ptr(), ws.data_ptr(), ops._stream())
    return out


def render_event_counts(cnt, round=False):
    """The pictures of count images: cnt [B,2,h,w] (fp32, on the GPU) -> uint8 [B,h,w,3] on the GPU, image b the array the
    reference's event_visualisation.plot_event_cnt returns for cnt[b].transpose(1, 2, 0) with its defaults (blue_red on white,
    normalised by the 1st / 99th percentiles; myutils/vis_events/matplotlib_plot_events.py:125-248), byte for byte -- what
    infer_BMCNet.py:90-97 hands matplotlib for lr_event_img, hr_bicubic_event_img, hr_esr_event_img and hr_gt_event_img.
    round=True rounds the counts half-to-even first, as :94 rounds the prediction.  bmc_slot_render on a temporary slot table
    (include/bmc_hip.h "event-count images" states the contract; 1 <= h * w <= 2^24, finite values)."""
    from . import slots
    if not (torch.is_tensor(cnt) and cnt.dim() == 4 and cnt.shape[1] == 2 and cnt.dtype == torch.float32):
        raise ValueError("render_event_counts: cnt must be an fp32 [B,2,h,w] tensor")
    B, _, h, w = cnt.shape
    if not 1 <= h * w <= slots.MAX_RENDER_PIXELS:
        raise ValueError("render_event_counts: images of 1 .. 2^24 pixels can be rendered (got %d x %d)" % (h, w))
    if not cnt.is_cuda:
        raise RuntimeError("render_event_counts: cnt must live on the MI355X (no CPU fallback in this build)")
    cnt = cnt.contiguous()
    out = torch.empty(B, h, w, 3, dtype=torch.uint8, device=cnt.device)
    scratch = torch.empty(4 * min(max(B, 1), slots.MAX_SLOTS), dtype=torch.float32, device=cnt.device)
    tables = {}
    for a in range(0, B, slots.MAX_SLOTS):
        n = min(slots.MAX_SLOTS, B - a)
        t = tables[n] = tables.get(n) or slots.SlotTable(n, cnt.device, render=1)
        e = t.host()
        rn = t.render_host()[0]
        for s in range(n):
            e[s]["frames"], e[s]["flags"] = cnt[a + s].data_ptr(), slots.ACTIVE
            rn[s]["src"], rn[s]["dst"] = cnt[a + s].data_ptr(), out[a + s].data_ptr()
        t.upload()
        slots.render(t, 0, h, w, round, scratch)
    return out


def counts_to_voxel(pred, bins, max_count=255):
    """The voxel grids of count images: pred [B,2,sH,sW] (fp32, on the GPU) -> float32 [B,bins,sH,sW] on the GPU, grid b what
    the reference's events_to_voxel_torch (dataloader/encodings.py:100-148, temporal bilinear) returns for the timed event
    stream of pred[b] -- events_to_voxel_torch(xs, ys, ts, ps, bins, sensor_size=(sH, sW)) of counts_to_events(pred[b:b+1],
    max_count, times="linear")'s columns as float32 --, bit for bit, without building the stream: per output pixel a closed form
    of its two counts (bmc_slot_voxel on a temporary slot table: two launches, no sort, no atomics; include/bmc_hip.h "voxel
    grids" states the contract).  The grid's rows are the sensor's y: vertically flipped against pred's rows, as the emitted ys
    are.  An image of 3 events or fewer gives zeros.  1 <= bins <= 32, 1 <= max_count <= 255."""
    import numpy as np
    from . import slots
    if not (torch.is_tensor(pred) and pred.dim() == 4 and pred.shape[1] == 2 and pred.dtype == torch.float32):
        raise ValueError("counts_to_voxel: pred must be an fp32 [B,2,sH,sW] tensor")
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= slots.MAX_VOXEL_BINS:
        raise ValueError("counts_to_voxel: bins must be an integer, 1 <= bins <= %d (got %r)" % (slots.MAX_VOXEL_BINS, bins))
    if isinstance(max_count, bool) or not isinstance(max_count, int) or not 1 <= max_count <= slots.MAX_COUNT_TIMED:
        raise ValueError("counts_to_voxel: max_count must be an integer, 1 <= max_count <= %d (the timed stream's limit; got %r)"
                         % (slots.MAX_COUNT_TIMED, max_count))
    B, _, sH, sW = pred.shape
    if not (1 <= sH <= slots.MAX_COUNT_LIMIT and 1 <= sW <= slots.MAX_COUNT_LIMIT):
        raise ValueError("counts_to_voxel: images of 1 .. %d pixels a side (got %d x %d)" % (slots.MAX_COUNT_LIMIT, sH, sW))
    if not pred.is_cuda:
        raise RuntimeError("counts_to_voxel: pred must live on the MI355X (no CPU fallback in this build)")
    pred = pred.contiguous()
    bins = int(bins)
    out = torch.empty(B, bins, sH, sW, dtype=torch.float32, device=pred.device)
    nparts = slots.voxel_parts(sH, sW)
    parts = torch.zeros(2 * min(max(B, 1), slots.MAX_SLOTS) * nparts, dtype=torch.int32, device=pred.device)
    tables = {}
    for a in range(0, B, slots.MAX_SLOTS):
        n = min(slots.MAX_SLOTS, B - a)
        t = tables[n] = tables.get(n) or slots.SlotTable(n, pred.device, voxel=True)
        e = t.host()
        vx = t.voxel_host()
        for s in range(n):
            e[s]["frames"], e[s]["flags"] = pred[a + s].data_ptr(), slots.ACTIVE
            vx[s]["dst"] = out[a + s].data_ptr()
        t.upload()
        slots.voxel(t, pred[a:a + n], max_count, bins, nparts, parts)
    return out


def image_quality(img, ref, data_range="gt", raw=False):
    """PSNR and SSIM of count images: img, ref [N,2,h,w] (fp32, on the GPU; h, w >= 7) -> dict(psnr=[N], ssim=[N]) numpy float64,
    image n what the reference's psnr_loss / ssim_loss (loss/restore.py:44-93: scikit-image's peak_signal_noise_ratio and
    structural_similarity per channel, the mean of the two) give for img[n] against the ground truth ref[n], in float64 on the
    float32 inputs: SSIM with the uniform 7x7 window, K1 = 0.01, K2 = 0.03 and sample covariance over the (h - 6) x (w - 6)
    window positions inside the image; data_range "gt": R_c = max(ref[n, c]) - min(ref[n]) (restore.py:85), or a positive
    constant.  IEEE results stand: psnr +inf for an exact channel, -inf for R_c = 0 with an error; ssim nan for R_c = 0.
    bmc_slot_quality on a temporary slot table (three launches, no atomics; include/bmc_hip_quality.h states the contract).
    raw=True: the dict also carries raw = [N, 2 channels, 4] float64, the kernels' records {sse, gt_max, gt_min, ssim_sum}."""
    from . import slots
    for name, t in (("img", img), ("ref", ref)):
        if not (torch.is_tensor(t) and t.dim() == 4 and t.shape[1] == 2 and t.dtype == torch.float32):
            raise ValueError("image_quality: %s must be an fp32 [N,2,h,w] tensor" % name)
    if img.shape != ref.shape:
        raise ValueError("image_quality: img %s and ref %s differ in shape" % (tuple(img.shape), tuple(ref.shape)))
    rng = slots.check_data_range("image_quality: ", data_range)
    N, _, h, w = img.shape
    if min(h, w) < slots.QUALITY_WIN or 2 * h * w >= 2 ** 30:
        raise ValueError("image_quality: images of at least %d x %d and fewer than 2^29 pixels (got %d x %d)"
                         % (slots.QUALITY_WIN, slots.QUALITY_WIN, h, w))
    if not (img.is_cuda and ref.is_cuda and img.device == ref.device):
        raise RuntimeError("image_quality: img and ref must live on the MI355X (no CPU fallback in this build)")
    img, ref = img.contiguous(), ref.contiguous()
    rec = torch.zeros(N, 2, slots.QUALITY_WORDS, dtype=torch.float64, device=img.device)
    most, nparts = min(max(N, 1), slots.MAX_SLOTS), slots.metric_parts(h, w)
    stats = torch.zeros(most * nparts * slots.QUALITY_STATS_WORDS, dtype=torch.float64, device=img.device)
    tiles = torch.zeros(most * 4 * slots.quality_tiles(h, w), dtype=torch.float64, device=img.device)
    tables = {}
    for a in range(0, N, slots.MAX_SLOTS):
        n = min(slots.MAX_SLOTS, N - a)
        t = tables[n] = tables.get(n) or slots.SlotTable(n, img.device, quality=True)
        e = t.host()
        qe = t.quality_host()
        for s in range(n):
            e[s]["frames"], e[s]["gt"], e[s]["flags"] = ref[a + s].data_ptr(), ref[a + s].data_ptr(), slots.ACTIVE
            qe[s]["dst"] = rec[a + s].data_ptr()
        t.upload()
        slots.quality(t, img[a:a + n], None, nparts, rng, stats, tiles)
    rec = rec.cpu().numpy()
    psnr, ssim = slots.quality_values(rec, data_range, (h, w))
    return dict(psnr=psnr, ssim=ssim, raw=rec) if raw else dict(psnr=psnr, ssim=ssim)


def counts_to_events(pred, max_count=255, times=None, spans=None, cuts=None):
    """The event stream of count images: pred [B,2,sH,sW] (fp32, on the GPU; e.g. what StreamingSR.step returns) ->
    (xs int16, ys int16, ps int8, index [B+1] int64 on the host); image b owns events [index[b], index[b+1]).  Per element v in
    the flat order of [2,sH,sW]: q = min(rint(v), max_count) for v > 0, else 0 (round-half-to-even: the rounded count image the
    reference renders, infer_BMCNet.py:94), q events xs = x, ys = sH-1-row, ps = +1 (channel 0) / -1 (channel 1) -- encoding
    image b's events at (sH, sW) without flips gives q back.  bmc_slot_emit on a temporary slot table, twice: a pass that only
    counts (capacity 0) sizes the columns and gives every image its start, the second pass writes.
    times="linear" (max_count <= 255): -> (xs, ys, ps, ts float32, index); event j of an element's n events has the time
    float32(0.01 + 0.99 * j / (n - 1)) (0.01 for n = 1) and every image's events are sorted by the exact j / (n - 1), ties in
    the flat order above -- the reference's linear redistribution (dataloader/encodings.py:367-414) with one time bin, by
    bmc_slot_emit_timed (include/bmc_hip.h states the contract).
    spans [B,2] (with times="linear"; float64 on the host): (t_first, t_last) of every image on the sensor's clock -> ts is
    FLOAT64 on that clock, t = t_first + tau * (t_last - t_first) with tau the float64 time above from the reduced fraction
    (bmc_slot_emit_clocked); events and order are the same.
    cuts [B] (with spans; float64 on the host, +inf allowed, no NaN): image b keeps exactly its events with ts < cuts[b] -- a
    prefix of its sorted events, the same bytes, trimmed before the sort (bmc_slot_emit_trimmed; include/bmc_hip_stream.h states
    the contract) -> (xs, ys, ps, ts, index, dropped): index counts the kept events, dropped [B] int64 on the host those cut off."""
    import numpy as np
    from . import slots, stream_lib
    if times not in (None, "linear"):
        raise ValueError("counts_to_events: times must be None or 'linear' (got %r)" % (times,))
    timed = times is not None
    if spans is not None and not timed:
        raise ValueError("counts_to_events: spans needs times='linear'")
    if not (torch.is_tensor(pred) and pred.dim() == 4 and pred.shape[1] == 2 and pred.dtype == torch.float32):
        raise ValueError("counts_to_events: pred must be an fp32 [B,2,sH,sW] tensor")
    if isinstance(max_count, bool) or not isinstance(max_count, int) or not 1 <= max_count <= slots.MAX_COUNT_LIMIT:
        raise ValueError("counts_to_events: max_count must be an integer, 1 <= max_count <= %d (got %r)"
                         % (slots.MAX_COUNT_LIMIT, max_count))
    if timed and max_count > slots.MAX_COUNT_TIMED:
        raise ValueError("counts_to_events: times='linear' needs max_count <= %d (got %d)" % (slots.MAX_COUNT_TIMED, max_count))
    if spans is not None:
        spans = check_spans("counts_to_events: ", spans, pred.shape[0])
    if cuts is not None:
        if spans is None:
            raise ValueError("counts_to_events: cuts needs spans (the clock the cut is made on)")
        cuts = np.asarray(cuts.cpu() if torch.is_tensor(cuts) else cuts)
        if cuts.shape != (pred.shape[0],) or cuts.dtype.kind not in "fiu":
            raise ValueError("counts_to_events: cuts must hold one number per image (got %s %s)" % (cuts.dtype, cuts.shape))
        cuts = cuts.astype(np.float64)
        if np.isnan(cuts).any():
            raise ValueError("counts_to_events: a cut must not be NaN")
    if not pred.is_cuda:
        raise RuntimeError("counts_to_events: pred must live on the MI355X (no CPU fallback in this build)")
    pred = pred.contiguous()
    B, _, sH, sW = pred.shape
    dev = pred.device
    clocked, trimmed = spans is not None, cuts is not None
    nparts = slots.emit_parts(sH, sW)
    groups = [(a, min(a + slots.MAX_SLOTS, B)) for a in range(0, B, slots.MAX_SLOTS)]
    tables = {b - a: slots.SlotTable(b - a, dev, emit=True, timed=timed, clock=clocked, trim=trimmed) for a, b in groups}
    parts = torch.zeros((stream_lib.TRIM_PARTS if trimmed else 1) * min(B, slots.MAX_SLOTS) * nparts, dtype=torch.int32, device=dev)
    dropped = torch.zeros(B, dtype=torch.int64, device=dev) if trimmed else None
    start = torch.zeros(B, dtype=torch.int64, device=dev)
    end = torch.zeros(B, dtype=torch.int64, device=dev)

    def run(xs, ys, ps, capacity, ts=None, window=1):
        scratch = None
        for a, b in groups:
            t = tables[b - a]
            e = t.host()
            em = t.emit_host()
            for s in range(b - a):
                e[s]["frames"], e[s]["flags"] = pred.data_ptr(), slots.ACTIVE
                em[s]["xs"], em[s]["ys"], em[s]["ps"] = xs.data_ptr(), ys.data_ptr(), ps.data_ptr()
                em[s]["index_in"], em[s]["index_out"] = start.data_ptr() + 8 * (a + s), end.data_ptr() + 8 * (a + s)
                em[s]["capacity"] = capacity
                if clocked:
                    ck = t.clock_host()
                    ck[s]["t_first"], ck[s]["t_last"], ck[s]["ts"] = spans[a + s, 0], spans[a + s, 1], ts.data_ptr()
                if trimmed:
                    tr = t.trim_host()
                    tr[s]["t_cut"], tr[s]["dropped"] = cuts[a + s], dropped.data_ptr() + 8 * (a + s)
                elif timed:
                    em[s]["ts"] = ts.data_ptr()
            t.upload()
            if timed:                                      # (the counting pass sorts nothing: window = 1, capacity = 0)
                if scratch is None:
                    scratch = torch.empty(slots.emit_timed_scratch_bytes(min(B, slots.MAX_SLOTS), nparts, window),
                                          dtype=torch.uint8, device=dev)
                emit = slots.emit_trimmed if trimmed else slots.emit_clocked if clocked else slots.emit_timed
                emit(t, pred[a:b], max_count, nparts, parts, scratch, window)
            else:
                slots.emit(t, pred[a:b], max_count, nparts, parts)

    none = (torch.empty(1, dtype=torch.int16, device=dev), torch.empty(1, dtype=torch.int16, device=dev),
            torch.empty(1, dtype=torch.int8, device=dev))
    ts_dtype = torch.float64 if clocked else torch.float32
    no_ts = torch.empty(1, dtype=ts_dtype, device=dev)
    run(*none, 0, no_ts)                                   # start = 0: end[b] = the events of image b; nothing is stored
    index = torch.zeros(B + 1, dtype=torch.int64)
    counts = end.cpu()
    index[1:] = counts.cumsum(0)
    total = int(index[B])
    if total == 0:
        return (none[0][:0], none[1][:0], none[2][:0]) + ((no_ts[:0],) if timed else ()) + (index,) + ((dropped.cpu(),) if trimmed else ())
    xs, ys = torch.empty(total, dtype=torch.int16, device=dev), torch.empty(total, dtype=torch.int16, device=dev)
    ps = torch.empty(total, dtype=torch.int8, device=dev)
    start.copy_(index[:B])
    if timed:
        ts = torch.empty(total, dtype=ts_dtype, device=dev)
        run(xs, ys, ps, total, ts, int(counts.max()))
        return (xs, ys, ps, ts, index) + ((dropped.cpu(),) if trimmed else ())
    run(xs, ys, ps, total)
    return xs, ys, ps, index


def encode_sequences(table, B, L, lr_size, gt_size, out=None):
    """The training batch of a DEVICE table of B bmc_seq_sample_t entries (uint8 tensor; event_dataset.SEQ_SAMPLE_DTYPE) ->
    (inp_cnt [B,L,2,H,W], gt_cnt [B,L,2,gh,gw]) float32: ONE bmc_seq_encode launch on the current stream (include/bmc_hip.h
    "sequence encoder for training").  The ranges of the table are trusted: event_dataset.EventTrainSet checks them when a
    recording is added.  Bit 3 of an entry's `flips` (transpose) is ignored here: full frames have one size per launch.
    out: (inp_cnt, gt_cnt) to write into instead of new tensors."""
    B, L = int(B), int(L)
    (H, W), (gh, gw) = (int(v) for v in lr_size), (int(v) for v in gt_size)
    if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.uint8 and table.is_contiguous()):
        raise RuntimeError("encode_sequences: the table must be a contiguous uint8 tensor on the MI355X (no CPU fallback in this build)")
    if B < 1 or table.numel() < B * SEQ_SAMPLE_BYTES or table.data_ptr() % 8:
        raise ValueError("encode_sequences: the table holds fewer than %d entries of %d bytes (8-byte aligned)" % (B, SEQ_SAMPLE_BYTES))
    shapes = ((B, L, 2, H, W), (B, L, 2, gh, gw))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.float32, device=table.device) for s in shapes)
    for t, s in zip(out, shapes):
        if not (t.is_cuda and t.device == table.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == s):
            raise ValueError("encode_sequences: out must be contiguous float32 tensors %s and %s on the table's device" % shapes)
    with torch.cuda.device(table.device):
        lib.call(lib._seq_encode, "bmc_seq_encode", table.data_ptr(), B, L, H, W, gh, gw, out[0].data_ptr(), out[1].data_ptr(),
                 ops._stream())
    return out[0], out[1]


def encode_sequence_crops(table, crops, B, L, crop, scale, out=None):
    """encode_sequences for patches: a DEVICE table of B bmc_seq_sample_t entries and, parallel to it, a DEVICE table of B
    bmc_seq_crop_t entries (uint8 tensors; event_dataset.SEQ_SAMPLE_DTYPE / SEQ_CROP_DTYPE) -> (inp_cnt [B,L,2,h,w], gt_cnt
    [B,L,2,scale*h,scale*w]) float32, crop = (h, w): ONE bmc_seq_encode_crop launch on the current stream (include/bmc_hip.h
    "sequence encoder for training").  Every sample is cut out of its own full frames, which may differ in size.  A sample
    with bit 3 of its entry's `flips` set is cut out of its TRANSPOSED frames -- full.transpose(-1, -2)[..., top:top+h,
    left:left+w], the origin in the transposed frames' rows / columns -- in the same launch; the crop entry keeps the
    recording's own (H, W, gh, gw).  The ranges and the crops are trusted: event_dataset.EventTrainSet checks them.
    out: (inp_cnt, gt_cnt) to write into."""
    B, L, scale = int(B), int(L), int(scale)
    h, w = (int(v) for v in crop)
    for name, t in (("table", table), ("crop table", crops)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise RuntimeError("encode_sequence_crops: the %s must be a contiguous uint8 tensor on the MI355X "
                               "(no CPU fallback in this build)" % name)
    if B < 1 or table.numel() < B * SEQ_SAMPLE_BYTES or table.data_ptr() % 8:
        raise ValueError("encode_sequence_crops: the table holds fewer than %d entries of %d bytes (8-byte aligned)"
                         % (B, SEQ_SAMPLE_BYTES))
    if crops.numel() < B * SEQ_CROP_BYTES or crops.data_ptr() % 8 or crops.device != table.device:
        raise ValueError("encode_sequence_crops: the crop table holds fewer than %d entries of %d bytes (8-byte aligned, on the "
                         "table's device)" % (B, SEQ_CROP_BYTES))
    shapes = ((B, L, 2, h, w), (B, L, 2, scale * h, scale * w))
    if out is None:
        if min(shapes[0] + shapes[1]) < 1:
            raise ValueError("encode_sequence_crops: B, L, crop and scale must be positive")
        out = tuple(torch.empty(s, dtype=torch.float32, device=table.device) for s in shapes)
    for t, s in zip(out, shapes):
        if not (t.is_cuda and t.device == table.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == s):
            raise ValueError("encode_sequence_crops: out must be contiguous float32 tensors %s and %s on the table's device" % shapes)
    with torch.cuda.device(table.device):
        lib.call(lib._seq_encode_crop, "bmc_seq_encode_crop", table.data_ptr(), crops.data_ptr(), B, L, h, w, scale,
                 out[0].data_ptr(), out[1].data_ptr(), ops._stream())
    return out[0], out[1]


SEQ_SAMPLE_BYTES = lib.STRUCTS["bmc_seq_sample_t"].size
SEQ_CROP_BYTES = lib.STRUCTS["bmc_seq_crop_t"].size
