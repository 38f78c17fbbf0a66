"""Plain restatements of the fused centre chain's two entry points, bmc_chain_fwd and bmc_chain_bwd, written from the contract
in include/bmc_hip.h ("fused centre chain of the BIE block"), not from csrc/chain.hip: torch on the CPU, no tiling, no rings.

  chain_fwd / chain_bwd    the operation itself, in float64 (the reference) or in float32 with one of two summation orders:
                           order="aten"   every dot product is one ATen matmul (F.linear), every mean one ATen mean;
                           order="serial" every dot product and every mean adds its terms one after the other in channel
                                          order, the dot products starting from their bias -- what a K-chained accumulator
                                          does at its worst.
                           The two float32 restatements are the yardsticks of tests/test_gpu_chain_kernels.py.
  hard_bound_fwd / _bwd    a first-order running error bound per output element, in float64, for ANY float32 evaluation of
                           the same formulas (u = 2^-24, round to nearest):
                             * a dot product of K terms plus bias, in any order:  (K + 1) u (sum |terms| + |bias|);
                             * a mean of C terms:  (C + 2) u mean |terms|  (C - 1 additions, the scaling, 1/C inexact);
                             * an elementwise operation:  u |result|;
                             * an error already present passes through a linear step as |W| bound and through the
                               LayerNorm and its backward step by step, every partial derivative taken in absolute value.
                           Loose on purpose (ATen's and the serial order's errors are 0.0005 .. 0.05 of it for every
                           output at C = 32 and 128, and 0.42 of it for rstd on constant rows, where the two roundings of
                           1/sqrt are all there is): a backstop no correct implementation crosses, not a measure of
                           sensitivity.
  launch_batches           the batch map and channel window of a bmc_src_t as plain indexing.

tests/test_chain_ref_cpu.py checks the float64 functions against torch autograd and both float32 orders against the bounds."""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
U = 2.0 ** -24
_CHUNK = 4096               # pixels per block of the serial dot product (the accumulator stays in cache)


def launch_batches(t, B, shift=0, mod=None, b0=0, c0=0, nch=None):
    """What launch batches 0 .. B-1 read of t [Bt,H,W,Ct] through a bmc_src_t: batch ((b + shift) % mod) + b0, channels
    [c0, c0 + nch).  mod None = B + shift (no wrap)."""
    mod = B + shift if mod is None else mod
    nch = t.shape[-1] - c0 if nch is None else nch
    return t[[(b + shift) % mod + b0 for b in range(B)]][..., c0:c0 + nch]


def _as(t, dtype):
    return None if t is None else torch.as_tensor(t).detach().to("cpu", dtype)


def _w2(w, dtype):
    w = _as(w, dtype)
    return w.reshape(w.shape[0], -1)          # a 1x1 convolution's [Cout, Cin, 1, 1] is its matrix


def _dot(x, w, start, dtype, order):
    """x [N,K], w [Cout,K], start [N,Cout] / [Cout] / None  ->  start + x w^T  [N,Cout]."""
    if dtype == F64 or order == "aten":
        y = F.linear(x, w)
        return y if start is None else start + y
    if order != "serial":
        raise ValueError("order: 'aten' or 'serial'")
    N, K = x.shape
    Cout = w.shape[0]
    wt = w.t().contiguous()
    out = torch.empty(N, Cout, dtype=dtype)
    for lo in range(0, N, _CHUNK):
        xt = x[lo:lo + _CHUNK].t().contiguous()               # [K, n]
        n = xt.shape[1]
        if start is None:
            acc = torch.zeros(n, Cout, dtype=dtype)
        else:
            acc = (start[lo:lo + _CHUNK] if start.dim() == 2 else start.expand(n, Cout)).clone()
        tmp = torch.empty_like(acc)
        for k in range(K):                                    # product rounded, then added: one term after the other
            torch.mul(xt[k].unsqueeze(1), wt[k].unsqueeze(0), out=tmp)
            acc.add_(tmp)
        out[lo:lo + _CHUNK] = acc
    return out


def _mean(v, dtype, order):
    """mean over the last axis, kept."""
    if dtype == F64 or order == "aten":
        return v.mean(-1, keepdim=True)
    vt = v.t().contiguous()                                   # [C, N]: a channel's values side by side
    acc = vt[0].clone()
    for c in range(1, vt.shape[0]):
        acc.add_(vt[c])
    return (acc / vt.shape[0]).unsqueeze(1)


def chain_fwd(s0, s1, Wf, bf, gamma, beta, Wc, bc, eps, dtype=F64, order="aten"):
    """s0, s1 [..., C] as the launch batches read them -> (yhat [..., C], rstd [...], centre [..., C]).
    z = Wf cat[s0, s1] + bf;  mu = mean_c z;  rstd = 1 / sqrt(mean_c (z - mu)^2 + eps);  yhat = (z - mu) rstd;
    centre = Wc (yhat gamma + beta) + bc.  eps is the entry point's float: it is rounded to float32 first."""
    lead, C = tuple(s0.shape[:-1]), s0.shape[-1]
    x = torch.cat([_as(s0, dtype).reshape(-1, C), _as(s1, dtype).reshape(-1, C)], 1)
    Wf, Wc, bf, bc, gamma, beta = _w2(Wf, dtype), _w2(Wc, dtype), _as(bf, dtype), _as(bc, dtype), _as(gamma, dtype), _as(beta, dtype)
    eps = torch.tensor(float(np.float32(eps)), dtype=dtype)
    z = _dot(x, Wf, bf, dtype, order)
    d = z - _mean(z, dtype, order)
    rstd = 1.0 / torch.sqrt(_mean(d * d, dtype, order) + eps)
    yhat = d * rstd
    centre = _dot(yhat * gamma + beta, Wc, bc, dtype, order)
    return yhat.reshape(lead + (C,)), rstd.reshape(lead), centre.reshape(lead + (C,))


def chain_bwd(dcentre, yhat, rstd, gamma, Wf, Wc, add, n, dtype=F64, order="aten"):
    """dcentre, yhat [2n,H,W,C], rstd [2n,H,W] (yhat and rstd as GIVEN: inputs, not recomputed), add [n,H,W,C] or None
    -> (dz [2n,H,W,C], ds1 [2n,H,W,C], ds0 [n,H,W,C]).
    dy = Wc^T dcentre;  g = dy gamma;  dz = rstd (g - yhat mean_c(g yhat) - mean_c(g));
    ds1[(bb + n) % 2n] = Wf[:, C:]^T dz[bb];  ds0[b] = add[b] + Wf[:, :C]^T (dz[b] + dz[b + n])."""
    shape, C = tuple(dcentre.shape), dcentre.shape[-1]
    assert shape[0] == 2 * n
    dc, yh = _as(dcentre, dtype).reshape(-1, C), _as(yhat, dtype).reshape(-1, C)
    rs = _as(rstd, dtype).reshape(-1, 1)
    Wf, Wc, gamma = _w2(Wf, dtype), _w2(Wc, dtype), _as(gamma, dtype)
    g = _dot(dc, Wc.t(), None, dtype, order) * gamma
    m2, m1 = _mean(g * yh, dtype, order), _mean(g, dtype, order)
    dz = rs * (g - yh * m2 - m1)
    ds1 = _dot(dz, Wf[:, C:].t(), None, dtype, order).reshape(shape)
    ds1 = torch.cat([ds1[n:], ds1[:n]])                       # batch bb's result lands at (bb + n) % 2n
    dz = dz.reshape(shape)
    half = (dz[:n] + dz[n:]).reshape(-1, C)
    start = None if add is None else _as(add, dtype).reshape(-1, C)
    ds0 = _dot(half, Wf[:, :C].t(), start, dtype, order).reshape((n,) + shape[1:])
    return dz, ds1, ds0


# ------------------------------------------------------------------ running error bounds (float64, first order)
def _dot_bound(x, w, start, e_x):
    """bound of start + x w^T given the bound e_x of x (start and w exact)."""
    K = x.shape[1]
    mag = F.linear(x.abs(), w.abs())
    if start is not None:
        mag = mag + start.abs()
    e = (K + 1) * U * mag
    return e if e_x is None else e + F.linear(e_x, w.abs())


def _mean_bound(v, e_v):
    C = v.shape[1]
    return e_v.mean(-1, keepdim=True) + (C + 2) * U * v.abs().mean(-1, keepdim=True)


def hard_bound_fwd(s0, s1, Wf, bf, gamma, beta, Wc, bc, eps):
    """-> bounds of (yhat, rstd, centre), shaped like chain_fwd's results."""
    lead, C = tuple(s0.shape[:-1]), s0.shape[-1]
    x = torch.cat([_as(s0, F64).reshape(-1, C), _as(s1, F64).reshape(-1, C)], 1)
    Wf, Wc, bf, bc, gamma, beta = _w2(Wf, F64), _w2(Wc, F64), _as(bf, F64), _as(bc, F64), _as(gamma, F64), _as(beta, F64)
    eps = float(np.float32(eps))
    z = F.linear(x, Wf, bf)
    e_z = _dot_bound(x, Wf, bf, None)
    mu = z.mean(-1, keepdim=True)
    d = z - mu
    e_d = e_z + _mean_bound(z, e_z) + U * d.abs()
    q = d * d
    e_q = 2 * d.abs() * e_d + U * q
    v = q.mean(-1, keepdim=True) + eps
    e_v = _mean_bound(q, e_q) + U * v
    rstd = 1.0 / torch.sqrt(v)
    e_r = 0.5 * rstd / v * e_v + 2 * U * rstd                 # the square root and the reciprocal
    yhat = d * rstd
    e_yh = rstd * e_d + d.abs() * e_r + U * yhat.abs()
    y = yhat * gamma + beta
    e_y = gamma.abs() * e_yh + U * (yhat * gamma).abs() + U * y.abs()
    e_c = _dot_bound(y, Wc, bc, e_y)
    return e_yh.reshape(lead + (C,)), e_r.reshape(lead), e_c.reshape(lead + (C,))


def hard_bound_bwd(dcentre, yhat, rstd, gamma, Wf, Wc, add, n):
    """-> bounds of (dz, ds1, ds0), shaped like chain_bwd's results."""
    shape, C = tuple(dcentre.shape), dcentre.shape[-1]
    dc, yh = _as(dcentre, F64).reshape(-1, C), _as(yhat, F64).reshape(-1, C)
    rs = _as(rstd, F64).reshape(-1, 1)
    Wf, Wc, gamma = _w2(Wf, F64), _w2(Wc, F64), _as(gamma, F64)
    dy = F.linear(dc, Wc.t())
    g = dy * gamma
    e_g = gamma.abs() * _dot_bound(dc, Wc.t(), None, None) + U * g.abs()
    p = g * yh
    e_p = yh.abs() * e_g + U * p.abs()
    m1, m2 = g.mean(-1, keepdim=True), p.mean(-1, keepdim=True)
    e_m1, e_m2 = _mean_bound(g, e_g), _mean_bound(p, e_p)
    t = yh * m2
    e_t = yh.abs() * e_m2 + U * t.abs()
    r = g - t - m1
    e_r = e_g + e_t + e_m1 + 2 * U * (g.abs() + t.abs() + m1.abs())      # two subtractions
    dz = rs * r
    e_dz = rs.abs() * e_r + U * dz.abs()
    W1t, W0t = Wf[:, C:].t(), Wf[:, :C].t()
    e_ds1 = _dot_bound(dz, W1t, None, e_dz).reshape(shape)
    e_ds1 = torch.cat([e_ds1[n:], e_ds1[:n]])
    dz4, e_dz4 = dz.reshape(shape), e_dz.reshape(shape)
    half = (dz4[:n] + dz4[n:]).reshape(-1, C)
    e_half = (e_dz4[:n] + e_dz4[n:]).reshape(-1, C) + U * half.abs()
    start = None if add is None else _as(add, F64).reshape(-1, C)
    e_ds0 = _dot_bound(half, W0t, start, e_half).reshape((n,) + shape[1:])
    return e_dz4, e_ds1, e_ds0


# ------------------------------------------------------------------ the pass rule and the input families of the two test files
def ulp32(m):
    m = abs(float(m))
    return float(np.spacing(np.float32(m))) if m != 0.0 else float(np.spacing(np.float32(0.0)))


def rule_b(got, ref, aten, serial):
    """The largest elementwise error of `got` over max(ATen-fp32 error, serial-fp32 error, 1 ulp of the largest output
    magnitude), every error taken against the same float64 `ref` -> (ratio, kernel, aten, serial, ulp).  The bar is 4."""
    got, ref, aten, serial = (_as(t, F64).reshape(-1) for t in (got, ref, aten, serial))
    ke, ae, se = (float((t - ref).abs().max()) for t in (got, aten, serial))
    floor = ulp32(ref.abs().max())
    return ke / max(ae, se, floor), ke, ae, se, floor


FWD_FAMILIES = ("plain", "lowvar", "mean1e3", "const")
BWD_FAMILIES = ("fwd", "synthetic")
EPS = 1e-6


def chain_params(C, g):
    """The parameter scales of the BIE test (tests/test_gpu_r2.py): weights randn / sqrt(fan-in), LayerNorm weight
    1 + 0.3 randn, everything else 0.1 randn."""
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(Wf=rn(C, 2 * C) / (2 * C) ** 0.5, bf=0.1 * rn(C), gamma=1.0 + 0.3 * rn(C), beta=0.1 * rn(C),
                Wc=rn(C, C) / C ** 0.5, bc=0.1 * rn(C))


def fwd_inputs(C, nb0, nb1, H, W, family, seed):
    """-> (s0 [nb0,H,W,C], s1 [nb1,H,W,C], parameters) in float32.
    plain    randn inputs, the parameter scales of the BIE test;
    lowvar   everything that feeds z (s0, s1, bf) scaled by 1e-3: the variance over channels is of the order of eps;
    mean1e3  bf shifted by 1e3: a large mean and a small spread;
    const    small-integer inputs, every row of Wf the same row of quarter-integers, bf constant: z is exact in any summation
             order and constant over a pixel's channels, so yhat = 0, rstd = 1/sqrt(eps), centre = Wc beta + bc."""
    g = torch.Generator().manual_seed(seed)
    p = chain_params(C, g)
    s0, s1 = torch.randn(nb0, H, W, C, generator=g), torch.randn(nb1, H, W, C, generator=g)
    if family == "lowvar":
        s0, s1, p["bf"] = s0 * 1e-3, s1 * 1e-3, p["bf"] * 1e-3
    elif family == "mean1e3":
        p["bf"] = p["bf"] + 1e3
    elif family == "const":
        s0 = torch.randint(-4, 5, (nb0, H, W, C), generator=g).float()
        s1 = torch.randint(-4, 5, (nb1, H, W, C), generator=g).float()
        p["Wf"] = (torch.randint(-3, 4, (1, 2 * C), generator=g).float() / 4).expand(C, 2 * C).contiguous()
        p["bf"] = torch.full((C,), 0.5)
    elif family != "plain":
        raise ValueError(family)
    return s0, s1, p


def bwd_inputs(C, n, H, W, family, seed):
    """-> (dcentre [2n,H,W,C], yhat [2n,H,W,C], rstd [2n,H,W], add [n,H,W,C], parameters) in float32.
    fwd        yhat and rstd are the float64 forward of plain inputs, rounded to float32;
    synthetic  yhat randn, rstd log-uniform in [0.5, 1e3]: large values beside ordinary ones."""
    g = torch.Generator().manual_seed(seed)
    if family == "fwd":
        s0, s1, p = fwd_inputs(C, 2 * n, 2 * n, H, W, "plain", seed + 1000)
        yhat, rstd, _ = chain_fwd(s0, s1, p["Wf"], p["bf"], p["gamma"], p["beta"], p["Wc"], p["bc"], EPS)
        yhat, rstd = yhat.float(), rstd.float()
    elif family == "synthetic":
        p = chain_params(C, g)
        yhat = torch.randn(2 * n, H, W, C, generator=g)
        rstd = 10.0 ** (torch.rand(2 * n, H, W, generator=g) * 3.3 - 0.3)
        rstd.view(-1)[0] = 1e3
    else:
        raise ValueError(family)
    dc, add = torch.randn(2 * n, H, W, C, generator=g), torch.randn(n, H, W, C, generator=g)
    return dc, yhat, rstd, add, p
