"""NumPy restatement of the event-count renderer's contract (include/bmc_hip.h "event-count images"): what the reference's
plot_event_cnt (myutils/vis_events/matplotlib_plot_events.py:125-248) returns with its defaults (color_scheme="blue_red",
use_opencv=False, is_black_background=False, is_norm=True), without calling np.percentile: sort, pick the four order
statistics, NumPy's two-branch lerp in float32, normalise, clip, colour.  tests/test_event_render_cpu.py holds it against the
goldens the reference's own function produced and against an np.percentile-based rendering.

percentile_ranks(n) restates how NumPy (2.x, method "linear") places a percentile of a FLOAT32 array: q/100 is formed in the
array's dtype (np.true_divide(q, float32(100))), so the virtual index (n - 1) * q is a float32 product, rounded once; the
neighbours are floor and floor + 1 (both the last element when the index reaches n - 1) and gamma = index - floor in float32."""
import numpy as np

F = np.float32
KINDS = ("lr", "bicubic", "esr", "gt")


def percentile_ranks(n):
    """-> ((k_lo, k_lo_next, gamma_lo), (k_hi, k_hi_next, gamma_hi)) for the 1st and the 99th percentile of n values."""
    out = []
    for q in (F(1) / F(100), F(99) / F(100)):
        vi = F(F(n - 1) * q)
        if vi >= F(n - 1):
            out.append((n - 1, n - 1, F(0)))
        else:
            k = int(np.floor(vi))
            out.append((k, k + 1, F(vi - F(k))))
    return tuple(out)


def lerp32(a, b, t):
    """numpy.lib._function_base_impl._lerp on float32 scalars: a + (b - a) * t, and b - (b - a) * (1 - t) for t >= 0.5."""
    a, b, t = F(a), F(b), F(t)
    d = F(b - a)
    r = F(a + F(d * t))
    if t >= F(0.5):
        r = F(b - F(d * F(F(1) - t)))
    return r


def channel_min_max(plane):
    """(1st percentile, 99th percentile) of a float32 plane, as float32 scalars."""
    v = np.sort(np.asarray(plane, F).ravel() + F(0))          # (+0: a -0.0 is a +0.0)
    (k0, k1, g0), (k2, k3, g1) = percentile_ranks(v.size)
    return lerp32(v[k0], v[k1], g0), lerp32(v[k2], v[k3], g1)


def colour(pos, neg, mins, maxs):
    """The normalisation, the clip and the colouring of two float32 planes [h,w] given their percentiles -> uint8 [h,w,3]."""
    mx = maxs[0] if maxs[0] > maxs[1] else maxs[1]
    ch = []
    for v, mn in ((pos, mins[0]), (neg, mins[1])):
        v = np.asarray(v, F)
        if mn != mx:
            v = ((v - F(mn)) / F(mx - mn)).astype(F)
        ch.append(np.clip(v, F(0), F(1)).astype(F))
    p, n = ch
    is_p = (p > 0) & ((n == 0) | (p >= n))
    is_n = ~is_p & (n > 0)
    one = np.ones(p.shape, np.float64)
    inv_p, inv_n = (F(1) - p).astype(np.float64), (F(1) - n).astype(np.float64)
    c0 = np.where(is_p, one, np.where(is_n, inv_n, one))
    c1 = np.where(is_p, inv_p, np.where(is_n, inv_n, one))
    c2 = np.where(is_p, inv_p, one)
    return np.stack([(c * 255.0).astype(np.uint8) for c in (c2, c1, c0)], axis=-1)     # BGR -> RGB: the last axis reversed


def render_np(cnt, round=False):
    """cnt [2,h,w] float32 (channel 0 positive, 1 negative) -> uint8 [h,w,3]; round: np.round (half to even) first."""
    cnt = np.asarray(cnt, F)
    assert cnt.ndim == 3 and cnt.shape[0] == 2 and cnt[0].size >= 1
    if round:
        cnt = np.round(cnt)
    mm = [channel_min_max(cnt[c]) for c in (0, 1)]
    return colour(cnt[0], cnt[1], (mm[0][0], mm[1][0]), (mm[0][1], mm[1][1]))


def render_percentile_np(cnt, round=False):
    """The same image with np.percentile for the four percentiles (what the reference calls)."""
    cnt = np.asarray(cnt, F)
    if round:
        cnt = np.round(cnt)
    mins = [np.percentile(cnt[c], 1) for c in (0, 1)]
    maxs = [np.percentile(cnt[c], 99) for c in (0, 1)]
    return colour(cnt[0], cnt[1], mins, maxs)
