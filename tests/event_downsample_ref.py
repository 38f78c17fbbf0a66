"""The integrate-and-fire event downsampler of include/bmc_hip_downsample.h restated twice, and the streams its tests run on.

downsample_seq      the contract as it reads (the oracle): one plain Python loop over the events and an array of accumulators.
downsample_grouped  an independent form: the counted events grouped by LR pixel with ONE stable argsort, every segment walked on
                    its own, the firing events put back in column order by their original index.  It exists to test the oracle
                    (and is what tools/time_downsample.py times on the host, for scale).
Both -> (xs int16, ys int16, ts float64, ps float64, acc): the output columns and the final accumulators, an int64 [h, w] array."""
import numpy as np


def lr_size(H, W, s):
    return -(-H // s), -(-W // s)


def counted(xs, ys, ps, H, W):
    xs, ys, ps = np.asarray(xs).astype(np.int64), np.asarray(ys).astype(np.int64), np.asarray(ps, np.float64)
    return (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H) & ((ps > 0) | (ps < 0))


def downsample_seq(xs, ys, ts, ps, H, W, s, T):
    xs, ys = np.asarray(xs).astype(np.int64), np.asarray(ys).astype(np.int64)
    ts, ps = np.asarray(ts, np.float64), np.asarray(ps, np.float64)
    h, w = lr_size(H, W, s)
    acc = np.zeros((h, w), np.int64)
    out = []
    for i, (x, y, p) in enumerate(zip(xs.tolist(), ys.tolist(), ps.tolist())):
        if not (0 <= x < W and 0 <= y < H and (p > 0 or p < 0)):
            continue
        q = (y // s, x // s)
        acc[q] += 1 if p > 0 else -1
        if acc[q] == T:
            out.append((i, 1.0))
            acc[q] = 0
        elif acc[q] == -T:
            out.append((i, -1.0))
            acc[q] = 0
    idx = np.array([i for i, _ in out], np.int64)
    return ((xs[idx] // s).astype(np.int16), (ys[idx] // s).astype(np.int16), ts[idx], np.array([p for _, p in out], np.float64), acc)


def downsample_grouped(xs, ys, ts, ps, H, W, s, T):
    xs, ys = np.asarray(xs).astype(np.int64), np.asarray(ys).astype(np.int64)
    ts, ps = np.asarray(ts, np.float64), np.asarray(ps, np.float64)
    h, w = lr_size(H, W, s)
    ok = counted(xs, ys, ps, H, W)
    key = np.where(ok, (ys // s) * w + xs // s, h * w)
    perm = np.argsort(key, kind="stable")
    skey = key[perm]
    fire = np.zeros(len(xs), np.int8)
    acc = np.zeros(h * w, np.int64)
    bounds = np.searchsorted(skey, np.arange(h * w + 1))
    for q in np.flatnonzero(np.diff(bounds)):
        seg = perm[bounds[q]:bounds[q + 1]]
        a = 0
        for i, up in zip(seg.tolist(), (ps[seg] > 0).tolist()):
            a += 1 if up else -1
            if abs(a) == T:
                fire[i] = 1 if a > 0 else -1
                a = 0
        acc[q] = a
    idx = np.flatnonzero(fire)
    return ((xs[idx] // s).astype(np.int16), (ys[idx] // s).astype(np.int16), ts[idx], fire[idx].astype(np.float64), acc.reshape(h, w))


def same(a, b):
    """Two results agree byte for byte, dtypes included (the accumulators, where both have them, too)."""
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def stream(H, W, n, s, seed=0, coherent=0.8, ignored=0.03, nan=True):
    """event_denoise_ref.stream (a drifting bar plus noise, ties in ts, about 1 % out of range on every side) with polarities that
    make LR pixels fire: a share `coherent` of the events takes the sign of its LR block's checkerboard colour, which swaps halfway
    through the stream (fires of both signs at every pixel), the rest stays random; a share `ignored` is +0.0, -0.0 or NaN (nan=False: +0.0 in its place, for recordings, whose polarities
    are -1, 0 or +1)."""
    import event_denoise_ref as N
    xs, ys, ts, ps = N.stream(H, W, n, 0.3, seed=seed)
    rng = np.random.default_rng(seed + 1)
    colour = np.where((xs.astype(np.int64) // s + ys.astype(np.int64) // s) % 2 == 0, 1.0, -1.0) * np.where(np.arange(n) < n // 2, 1.0, -1.0)
    ps = np.where(rng.random(n) < coherent, colour, ps)
    kind = np.where(rng.random(n) < ignored, rng.integers(0, 3, n), -1)
    ps = np.where(kind == 0, 0.0, np.where(kind == 1, -0.0, np.where(kind == 2, np.nan if nan else 0.0, ps)))
    return xs, ys, ts, ps


# ------------------------------------------------------------------ planted streams: (xs, ys, ps) lists on one HR pixel (x, y)
def hysteresis_no_fire(T, x=0, y=0):
    """T-1 ups, one down, one up: the sum never reaches T."""
    ps = [1.0] * (T - 1) + [-1.0, 1.0]
    return [x] * len(ps), [y] * len(ps), ps


def exact_fire(T, x=0, y=0, sign=1.0):
    """Exactly T like-signed events, then T-1 more: one fire at event T-1, a reset, and no second fire."""
    ps = [sign] * (2 * T - 1)
    return [x] * len(ps), [y] * len(ps), ps


def alternating(n, x=0, y=0):
    ps = [1.0 if i % 2 == 0 else -1.0 for i in range(n)]
    return [x] * n, [y] * n, ps


def columns(xs, ys, ps, ts=None):
    """Lists -> the four columns; ts defaults to a 1e-6 tick per event."""
    n = len(xs)
    ts = np.arange(n, dtype=np.float64) * 1e-6 if ts is None else np.asarray(ts, np.float64)
    return np.asarray(xs, np.int16), np.asarray(ys, np.int16), ts, np.asarray(ps, np.float64)
