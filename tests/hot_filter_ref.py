"""The numpy restatement of the hot-pixel filter (include/bmc_hip.h, "hot-pixel filter", rules 1-5), shared by
test_hot_filter_cpu.py and test_gpu_hot_filter.py: what bmc_hot_pixel_mask, bmc_slot_hot_update and bmc_slot_encode_filtered must
produce byte for byte.  get_hot_event_mask_np is the reference's loop restated line by line (it is checked against the
reference's own outputs in tests/golden/hot_filter.npz); mask_from_counts_np is the integer form the kernel evaluates."""
import numpy as np

from oracle import bmc_oracle as O


def get_hot_event_mask_np(event_rate, idx, max_px=100, min_obvs=5, max_rate=0.8):
    """dataloader/encodings.py:349-364 on a float32 [H,W] array -> (mask float32 [H,W], event_rate after the call).  torch.argmax
    and np.argmax agree: the first maximum, a NaN counts as the maximum, -0.0 == +0.0.  torch compares a float32 element with the
    Python scalar in float32."""
    rate = np.array(event_rate, dtype=np.float32, copy=True)
    mask = np.ones(rate.shape, np.float32)
    thr = np.float32(max_rate)
    if idx > min_obvs:
        flat = rate.reshape(-1)
        for _ in range(int(max_px)):
            a = int(np.argmax(flat))
            if mask.reshape(-1)[a] == 0 and flat[a] == 0 and not np.signbit(flat[a]):
                break                                                # max_rate < 0: the loop re-finds an entry it zeroed -- a fixed point
            if flat[a] > thr:
                flat[a] = 0
                mask.reshape(-1)[a] = 0
            else:
                break
    return mask, rate


def cmin_np(idx, max_rate):
    """The smallest c in [0, idx] with float32(c) / float32(idx) > float32(max_rate); idx + 1 if there is none (brute force)."""
    c = np.arange(idx + 1)
    above = c.astype(np.float32) / np.float32(idx) > np.float32(max_rate)
    return int(np.argmax(above)) if above.any() else idx + 1


def mask_from_counts_np(count, idx, max_px, min_obvs, max_rate):
    """Rule 3 on the integers -> mask uint8 [H,W] (1 = keep): the pixels with count >= cmin, at most max_px of them, the largest
    counts first and equal counts in flat order; for max_rate < 0 the pixels with count >= 1 and, if fewer than max_px of them
    exist, pixel (0, 0) as well."""
    count = np.asarray(count, np.int64)
    flat = count.reshape(-1)
    mask = np.ones(flat.shape, np.uint8)
    if idx > min_obvs and max_px > 0:
        neg = np.float32(max_rate) < 0
        cmin = 1 if neg else cmin_np(idx, max_rate)
        cand = np.flatnonzero(flat >= cmin)
        order = cand[np.argsort(-flat[cand], kind="stable")]         # descending counts, ties in flat order
        mask[order[:max_px]] = 0
        if neg and len(cand) < max_px:
            mask[0] = 0
    return mask.reshape(count.shape)


def observe_np(xs, ys, ps, size):
    """Rule 1: obs [H,W] int32 (0 / 1) of one item's LR events (int16, int16, float64 columns)."""
    m = O.events_to_mask_np(np.asarray(xs).astype(np.float32), np.asarray(ys).astype(np.float32),
                            np.asarray(ps).astype(np.float32), size)[0]
    assert np.isin(m, (0, 1)).all()
    return m.astype(np.int32)


def filter_recording_np(lr, lr_index, size, max_px, min_obvs, max_rate):
    """Rules 1-4 for one recording: lr = (xs, ys, ps) columns, lr_index [L,2] -> dict(frames [L,2,H,W] float32 the filtered
    count images, raw [L,2,H,W] the unfiltered ones, masks [L,H,W] uint8 (sensor coordinates, 1 = keep), counts [L,H,W] int32
    (after item j), hot [L] the number of masked pixels).  The mask is the reference's own function on float32(count) /
    float32(idx) (rule 3's definition)."""
    xs, ys, ps = (np.asarray(c) for c in lr)
    H, W = size
    L = len(lr_index)
    out = dict(frames=np.zeros((L, 2, H, W), np.float32), raw=np.zeros((L, 2, H, W), np.float32),
               masks=np.ones((L, H, W), np.uint8), counts=np.zeros((L, H, W), np.int32), hot=np.zeros(L, np.int64))
    count = np.zeros((H, W), np.int32)
    for j, (a, b) in enumerate(np.asarray(lr_index)):
        count = count + observe_np(xs[a:b], ys[a:b], ps[a:b], size)
        idx = j + 1
        mask = get_hot_event_mask_np(count.astype(np.float32) / np.float32(idx), idx, max_px, min_obvs, max_rate)[0].astype(np.uint8)
        assert np.array_equal(mask, mask_from_counts_np(count, idx, max_px, min_obvs, max_rate)), (j, "integer form")
        raw = O.encode_raw_frame_np(xs[a:b], ys[a:b], ps[a:b], 0, size)
        out["raw"][j] = raw
        out["frames"][j] = raw * mask[::-1][None].astype(np.float32)  # rule 4: [H-1-y][x] of both channels
        out["masks"][j], out["counts"][j], out["hot"][j] = mask, count, int((mask == 0).sum())
    return out


def planted_recording(rng, size, L, n_events, hot, oob=4, empty_item=None, zero_last=None):
    """A small event-backed LR stream with planted hot pixels -> ((xs int16, ys int16, ps float64), lr_index [L,2]).
    Every item has n_events random events, `oob` out-of-range ones, then one event on every hot pixel (y, x) in `hot` -- so the
    hot pixels have equal counts.  empty_item: that item has no events.  zero_last = (item, k): that item ends with a p = 0
    event on hot pixel k (its observation there is 0)."""
    H, W = size
    xs, ys, ps, index = [], [], [], []
    n = 0
    for j in range(L):
        first = n
        if j != empty_item:
            x = rng.integers(0, W, n_events); y = rng.integers(0, H, n_events); p = rng.choice([-1.0, 1.0], n_events)
            ox = rng.choice([-1, W, W + 3], oob); oy = rng.integers(-2, H + 2, oob); op = rng.choice([-1.0, 1.0], oob)
            hy = np.array([h[0] for h in hot], np.int64); hx = np.array([h[1] for h in hot], np.int64)
            hp = rng.choice([-1.0, 1.0], len(hot))
            parts = [(x, y, p), (hx, hy, hp), (ox, oy, op)] if j % 2 else [(x, y, p), (ox, oy, op), (hx, hy, hp)]
            if zero_last is not None and zero_last[0] == j:
                k = zero_last[1]
                parts.append((hx[k:k + 1], hy[k:k + 1], np.zeros(1)))
            for a, b, c in parts:
                xs.append(a); ys.append(b); ps.append(c)
                n += len(a)
        index.append((first, n))
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
    return (cat(xs, np.int16), cat(ys, np.int16), cat(ps, np.float64)), np.array(index, np.int64)
