"""Plain float64 restatements of the HBM-bound streaming entry points of include/bmc_hip.h ("streaming kernels", "head / tail
of a recurrent window", "loss-side resize", bmc_chain_affine_grads), one function per entry point, written from the header's
contract: torch float64 on the CPU, no tiling, no fixed summation order.  The ops that only move or select data keep the dtype
of their input, so their results can be compared bit for bit.  tests/test_streaming_ref_cpu.py checks every function here
against what torch itself computes; tests/test_gpu_streaming_kernels.py checks the kernels against these functions."""
import functools

import torch

F64 = torch.float64


def _d(t):
    return None if t is None else t.detach().to("cpu", F64)


# ------------------------------------------------------------------ elementwise / sums
def relu_bwd(dy, y):
    """g = y > 0 ? dy : 0 (dtype of dy: a selection, bit-exact)."""
    return torch.where(y > 0, dy, torch.zeros_like(dy))


def group_sum(x, groups):
    """out[i] = sum_{k < groups} x[k*n + i] in float64; x flat [groups*n]."""
    return _d(x).reshape(groups, -1).sum(0)


def group_sum_f32(x, groups):
    """The same in float32, added in the contract's fixed order k = 0 .. groups-1: the op is bit-reproducible."""
    x = x.detach().to("cpu", torch.float32).reshape(groups, -1)
    s = x[0].clone()
    for k in range(1, groups):
        s = s + x[k]
    return s


def colsum(x, npix, pix_stride, C, prior=None, accumulate=0):
    """out[c] (+)= sum_p x[p*pix_stride + c]; x is the flat buffer the pointer addresses."""
    win = torch.as_strided(x.detach().cpu().reshape(-1), (npix, C), (pix_stride, 1))
    s = win.to(F64).sum(0)
    return s + _d(prior) if accumulate else s


# ------------------------------------------------------------------ LayerNorm2d over channels per pixel
def layernorm_fwd(x, gamma, beta, eps):
    """x [npix, C] -> y [npix, C], stats [npix, 2] = (mean, rstd); biased variance, eps inside the sqrt."""
    x, gamma, beta = _d(x), _d(gamma), _d(beta)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mu) * rstd * gamma + beta, torch.cat([mu, rstd], -1)


def layernorm_bwd(dy, x, stats, gamma, prior_dgamma=None, prior_dbeta=None, accumulate=0):
    """dx = rstd * (g - yhat*mean_c(g*yhat) - mean_c(g)), g = dy*gamma, yhat = (x - mean)*rstd with the (mean, rstd) given in
    stats (an input of the entry point); dgamma (+)= sum_p dy*yhat, dbeta (+)= sum_p dy."""
    dy, x, stats, gamma = _d(dy), _d(x), _d(stats), _d(gamma)
    mu, rstd = stats[:, 0:1], stats[:, 1:2]
    yhat = (x - mu) * rstd
    g = dy * gamma
    dx = rstd * (g - yhat * (g * yhat).mean(-1, keepdim=True) - g.mean(-1, keepdim=True))
    dgamma, dbeta = (dy * yhat).sum(0), dy.sum(0)
    if accumulate:
        dgamma, dbeta = dgamma + _d(prior_dgamma), dbeta + _d(prior_dbeta)
    return dx, dgamma, dbeta


# ------------------------------------------------------------------ row softmax
def softmax_fwd(a):
    a = _d(a)
    e = torch.exp(a - a.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_bwd(p, dp, scale_out=1.0):
    """dA = P * (dP - rowsum(dP*P)) * scale_out, P as given."""
    p, dp = _d(p), _d(dp)
    return p * (dp - (dp * p).sum(-1, keepdim=True)) * float(scale_out)


# ------------------------------------------------------------------ input packing
def pack_inputs(x, repeat):
    """x [B,2,T,H,W] with any strides (only frames 0 and 1 are read) -> (xin_p, xin_n) [B,H,W,16]: channels
    [f1]*repeat + [f2]*repeat + zeros of polarity 0 / 1.  Dtype of x (a copy, bit-exact)."""
    x = x.detach().cpu()
    B, _, _, H, W = x.shape
    out = []
    for pol in (0, 1):
        o = torch.zeros((B, H, W, 16), dtype=x.dtype)
        for k in range(repeat):
            o[..., k] = x[:, pol, 0]
            o[..., repeat + k] = x[:, pol, 1]
        out.append(o)
    return out[0], out[1]


# ------------------------------------------------------------------ pixel (un)shuffle, head
def _split_groups(lr, split):
    """[B,H,W,CC] -> [S*B,H,W,CC/S]: group s of sample b at batch s*B + b."""
    B, H, W, CC = lr.shape
    return lr.reshape(B, H, W, split, CC // split).permute(3, 0, 1, 2, 4).reshape(split * B, H, W, CC // split)


def _merge_groups(lr, split):
    SB, H, W, cg = lr.shape
    B = SB // split
    return lr.reshape(split, B, H, W, cg).permute(1, 2, 3, 0, 4).reshape(B, H, W, split * cg)


def unshuffle_to_nhwc(hr, r, split=1):
    """HR NCHW [B,C,rH,rW] -> LR NHWC [S*B,H,W,C*r*r/S], LR channel c*r*r + i*r + j <- HR (c, y*r+i, x*r+j).  Dtype of hr."""
    hr = hr.detach().cpu()
    B, C, HH, WW = hr.shape
    H, W = HH // r, WW // r
    lr = hr.reshape(B, C, H, r, W, r).permute(0, 2, 4, 1, 3, 5).reshape(B, H, W, C * r * r)
    return _split_groups(lr, split).contiguous()


def bilinear_up(base, r):
    """F.interpolate(base, scale_factor=r, mode='bilinear', align_corners=False) in float64: src = max((dst+0.5)/r - 0.5, 0),
    i0 = floor(src), i1 = min(i0+1, n-1), weight src - i0 on i1.  Returns (image, is_border_row [rH], is_border_col [rW]):
    the rows / columns whose taps meet one of the two clamps."""
    base = _d(base)
    H, W = base.shape[-2:]

    def axis(n):
        dst = torch.arange(n * r, dtype=F64)
        raw = (dst + 0.5) / r - 0.5
        src = raw.clamp(min=0.0)
        i0 = src.floor().long()
        i1 = (i0 + 1).clamp(max=n - 1)
        return i0, i1, src - i0, (raw < 0) | (i0 + 1 > n - 1)

    y0, y1, ly, by = axis(H)
    x0, x1, lx, bx = axis(W)
    ly = ly.view(-1, 1)
    top = base[..., y0, :][..., x0] * (1 - lx) + base[..., y0, :][..., x1] * lx
    bot = base[..., y1, :][..., x0] * (1 - lx) + base[..., y1, :][..., x1] * lx
    return top * (1 - ly) + bot * ly, by, bx


def shuffle_to_hr(lr, r, split=1, base=None):
    """LR NHWC [S*B,H,W,C*r*r/S] -> HR NCHW [B,C,rH,rW] (+ bilinear x r of base [B,C,H,W]).  Without base: dtype of lr
    (a permutation, bit-exact); with base: float64."""
    lr = _merge_groups(lr.detach().cpu(), split)
    B, H, W, CC = lr.shape
    C = CC // (r * r)
    hr = lr.reshape(B, H, W, C, r, r).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H * r, W * r).contiguous()
    if base is None:
        return hr
    return hr.to(F64) + bilinear_up(base, r)[0]


def head_mse_fwd(lr, base, gt, r):
    """pred = pixel_shuffle(lr, r) + bilinear(base), loss = mean((pred - gt)^2)."""
    pred = shuffle_to_hr(lr, r, 1, base)
    return pred, ((pred - _d(gt)) ** 2).mean()


def head_mse_bwd(dpred, pred, gt, gloss, r):
    """dlr = pixel_unshuffle(dpred + (2 gloss / numel) (pred - gt)); dpred / gloss None = that gradient is absent."""
    ref = pred if pred is not None else dpred
    g = torch.zeros(tuple(ref.shape), dtype=F64)
    if dpred is not None:
        g = g + _d(dpred)
    if gloss is not None:
        g = g + (2.0 * float(_d(gloss)) / g.numel()) * (_d(pred) - _d(gt))
    return unshuffle_to_nhwc(g, r, 1)


# ------------------------------------------------------------------ bicubic resize (ATen: A = -0.75, align_corners=False)
def bicubic_axis_matrix(n_in, n_out):
    """[n_out, n_in] float64: row dst holds the four cubic-convolution weights of src = (n_in/n_out)*(dst+0.5) - 0.5 on taps
    floor(src)-1 .. floor(src)+2, tap indices clamped to [0, n_in-1] (clamped taps add up)."""
    A = -0.75
    scale = n_in / n_out
    M = torch.zeros((n_out, n_in), dtype=F64)
    for dst in range(n_out):
        src = scale * (dst + 0.5) - 0.5
        i0 = int(torch.tensor(src, dtype=F64).floor())
        t = src - i0
        inner = lambda v: ((A + 2.0) * v - (A + 3.0)) * v * v + 1.0                      # |v| <= 1
        outer = lambda v: ((A * v - 5.0 * A) * v + 8.0 * A) * v - 4.0 * A                # 1 < |v| < 2
        w = (outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t))
        for k in range(4):
            M[dst, min(max(i0 - 1 + k, 0), n_in - 1)] += w[k]
    return M


@functools.lru_cache(maxsize=1)
def bicubic_matrix(H, W, Ho, Wo):
    """The forward operator of one plane as a dense [Ho*Wo, H*W] matrix (rows / columns in row-major pixel order)."""
    return torch.kron(bicubic_axis_matrix(H, Ho), bicubic_axis_matrix(W, Wo))


def bicubic_resize_fwd(x, Ho, Wo, dense=True):
    """x [planes, H, W] -> [planes, Ho, Wo]: the dense matrix times each plane (dense=False: the same operator applied
    axis by axis, for planes too large for the dense matrix)."""
    x = _d(x)
    P, H, W = x.shape
    if dense:
        return (x.reshape(P, H * W) @ bicubic_matrix(H, W, Ho, Wo).T).reshape(P, Ho, Wo)
    return bicubic_axis_matrix(H, Ho) @ x @ bicubic_axis_matrix(W, Wo).T


def bicubic_resize_bwd(gy, H, W, dense=True):
    """gy [planes, Ho, Wo] -> gx [planes, H, W]: the explicit transpose of the forward operator."""
    gy = _d(gy)
    P, Ho, Wo = gy.shape
    if dense:
        return (gy.reshape(P, Ho * Wo) @ bicubic_matrix(H, W, Ho, Wo)).reshape(P, H, W)
    return bicubic_axis_matrix(H, Ho).T @ gy @ bicubic_axis_matrix(W, Wo)


# ------------------------------------------------------------------ LayerNorm affine gradients of the fused centre chain
def chain_affine_grads(G, dbc, Wc, gamma, beta, prior=None, accumulate=0, want_dbc_out=False):
    """dwc[co][ci] (=|+=) gamma[ci] G[co][ci] + dbc[co] beta[ci];  dgamma[ci] (=|+=) sum_co Wc[co][ci] G[co][ci];
    dbeta (=|+=) Wc^T dbc;  dbc_out (=|+=) dbc.  prior = (dwc, dbc_out or None, dgamma, dbeta) before the call."""
    G, dbc, Wc, gamma, beta = _d(G), _d(dbc), _d(Wc), _d(gamma), _d(beta)
    dwc = gamma.view(1, -1) * G + dbc.view(-1, 1) * beta.view(1, -1)
    dgamma = (Wc * G).sum(0)
    dbeta = Wc.T @ dbc
    out = [dwc, dbc.clone() if want_dbc_out else None, dgamma, dbeta]
    if accumulate:
        out = [None if o is None else o + _d(p) for o, p in zip(out, prior)]
    return tuple(out)
