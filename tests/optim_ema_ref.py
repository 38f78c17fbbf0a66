"""The weight EMA of bmc_hip.optim.Adam(ema_decay=, ema_warmup=) restated without the GPU (include/bmc_hip_ema.h): the three
float32 lines in numpy (numpy never fuses a multiply into an add), the decay schedule in float64, a float64 EMA, and the error
bar between the two, derived here from the roundings -- not from anything a GPU produced.

The bar.  With u = 2^-24 and W = 1 - decay_t exact in float64, one float32 update computes
    w  = W (1 + a)                 the weight, rounded once
    d  = (p - e)(1 + b)            s = w d (1 + c)            e' = (e + s)(1 + f)            |a|, |b|, |c|, |f| <= u
so e' differs from the exact map e + W (p - e) of the SAME e by at most about 3 u |s| + u |e'|, plus 2^-149 when w * d underflows
(float32 sums and differences that land among the subnormals are exact).  The exact map is a contraction in e (factor 1 - W <= 1),
so an error already in e is not amplified; it only enters the magnitudes |s| and |e'| of the next update, a term of at most
4 u times the error.  Hence, per element, with s64 and e64 the float64 trajectory,
    bar_0 = 0        bar_k = bar_(k-1) (1 + 4 u) + u (3 |s64_k| + |e64_k|) + 2^-149
which bounds |e32_k - e64_k| after k updates."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149


def decay_at(decay, warmup, t):
    """decay_t of the step whose 1-based count is t: float64 operations only, each exactly rounded."""
    t = np.float64(t)
    return min(np.float64(decay), t / (t + np.float64(9.0))) if warmup else np.float64(decay)


def weight64(decay, warmup, t):
    return np.float64(1.0) - decay_at(decay, warmup, t)


def weight32(decay, warmup, t):
    """w: the float64 difference rounded to float32 once."""
    return np.float32(weight64(decay, warmup, t))


def ema32(e, p, w):
    """The three lines on float32 arrays, every operation rounded to float32 once."""
    assert e.dtype == np.float32 and p.dtype == np.float32 and type(w) is np.float32
    with np.errstate(all="ignore"):
        d = p - e
        s = w * d
        out = e + s
    assert d.dtype == s.dtype == out.dtype == np.float32
    return out


class Ema64:
    """The float64 EMA of a sequence of (float32) weights, with the bar of the float32 one beside it."""

    def __init__(self, p0):
        self.e = np.asarray(p0, dtype=np.float64).copy()
        self.bar = np.zeros_like(self.e)
        self.updates = 0

    def update(self, p, decay, warmup, t):
        W = weight64(decay, warmup, t)
        with np.errstate(all="ignore"):
            s = W * (np.asarray(p, dtype=np.float64) - self.e)
            self.e = self.e + s
            self.bar = self.bar * (1.0 + 4.0 * U) + U * (3.0 * np.abs(s) + np.abs(self.e)) + TINY
        self.updates += 1
        return self.e


def same_bits(a, b):
    """float32 arrays equal bit for bit, except that any NaN equals any NaN (sign and payload of a NaN are not compared)."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    nan = np.isnan(b)
    return bool(np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan]))
