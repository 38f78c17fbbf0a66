"""The background-activity noise filter of include/bmc_hip_denoise.h restated twice, and the streams its tests run on.

mask_seq     the contract as it reads: one plain Python loop over a numpy surface of latest event indices.
mask_sorted  a vectorised torch form for any device: ONE sort of the composite key pixel * n + index of the in-range events; the
             latest earlier event at neighbour pixel q of event i is the predecessor of the key q * n + i (searchsorted), once per
             neighbour.  The obvious composition on the GPU: what tools/time_denoise.py times the kernel against.
stream       a two-pixel bar drifting across the sensor plus uniform noise, timestamps on a 1e-6 tick (ties occur), about 1 % of
             the events out of range, on every side."""
import numpy as np
import torch

NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))      # (dy, dx)


def mask_seq(xs, ys, ts, H, W, dt, support):
    """-> keep uint8 [n].  xs, ys integer arrays, ts float64, non-decreasing."""
    xs, ys, ts = np.asarray(xs).astype(np.int64), np.asarray(ys).astype(np.int64), np.asarray(ts, np.float64)
    n = len(xs)
    last = np.full((H + 2, W + 2), -1, np.int64)             # a border of "none" around the sensor
    keep = np.zeros(n, np.uint8)
    tl = ts.tolist()
    dt = float(dt)
    for i, (x, y) in enumerate(zip(xs.tolist(), ys.tolist())):
        if not (0 <= x < W and 0 <= y < H):
            continue
        c = 0
        for dy, dx in NEIGHBOURS:
            j = last[y + 1 + dy, x + 1 + dx]
            if j >= 0 and tl[i] - tl[j] <= dt:               # one float64 subtraction, then the comparison
                c += 1
        keep[i] = c >= support
        last[y + 1, x + 1] = i
    return keep


def mask_sorted(xs, ys, ts, H, W, dt, support, stats=None):
    """-> keep uint8 [n], torch tensors on the device of xs.  stats (a dict): gets "temporary_bytes", the bytes of the n-sized
    temporaries alive at the peak (the keys, their sorted copy, the query, the positions, the predecessors, the counts)."""
    n, dev = xs.numel(), xs.device
    x, y = xs.to(torch.int64), ys.to(torch.int64)
    inr = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    key = ((y * W + x) * n + idx)[inr]
    key = torch.sort(key, stable=True).values
    c = torch.zeros(n, dtype=torch.int64, device=dev)
    if key.numel():
        for dy, dx in NEIGHBOURS:
            qy, qx = y + dy, x + dx
            ok = inr & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            q = torch.where(ok, qy * W + qx, torch.zeros_like(qy))
            pos = torch.searchsorted(key, q * n + idx)       # the key itself is absent: event i sits at another pixel
            prev = key[(pos - 1).clamp_(min=0)]
            ok &= (pos > 0) & (torch.div(prev, n, rounding_mode="floor") == q)
            j = prev % n
            c += ok & (ts - ts[j] <= dt)
    if stats is not None:
        stats["temporary_bytes"] = 8 * (6 * n + 2 * int(key.numel())) + 2 * n
    return (inr & (c >= support)).to(torch.uint8)


def stream(H, W, n, noise=0.3, seed=0, duration=1.0, oob=0.01):
    """-> xs int16, ys int16, ts float64 (sorted, on a 1e-6 tick), ps float64 (+-1) of n events: a share `noise` uniform over
    the sensor, the rest on a bar two pixels wide over all rows that crosses the sensor once in `duration`; a share `oob` of all
    events is moved out of range, a quarter of it past each side."""
    rng = np.random.default_rng(seed)
    ts = np.round(np.sort(rng.random(n)) * duration * 1e6) / 1e6
    is_noise = rng.random(n) < noise
    bar = np.floor(ts / duration * max(W - 1, 1)).astype(np.int64) + rng.integers(0, 2, n)
    xs = np.where(is_noise, rng.integers(0, W, n), np.minimum(bar, W - 1))
    ys = rng.integers(0, H, n)
    side = np.where(rng.random(n) < oob, rng.integers(0, 4, n), -1)
    far = rng.integers(0, 3, n)
    xs = np.where(side == 0, -1 - far, np.where(side == 1, W + far, xs))
    ys = np.where(side == 2, -1 - far, np.where(side == 3, H + far, ys))
    ps = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return xs.astype(np.int16), ys.astype(np.int16), ts.astype(np.float64), ps


# The generated cases: (H, W, n) -> (dt, the supports tested).  Each asserts on mask_seq's own output that both outcomes occur.
CASES = {(1, 9, 200): 2e-2, (5, 7, 600): 2e-2, (37, 53, 6000): 1e-2, (64, 96, 20000): 5e-3, (180, 240, 100000): 2e-3}


def both_outcomes(keep, n, dense=False):
    """The kept share lies in [0.05, 0.95] (n >= 200); dense (support 8): only that both outcomes occur."""
    k = int(np.asarray(keep).sum())
    if dense or n < 200:
        return 0 < k < n if n >= 200 else True
    return 0.05 <= k / n <= 0.95
