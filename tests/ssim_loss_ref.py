"""The structural loss 1 - mean SSIM and its gradient in float64: the oracle of bmc_ssim_loss_fwd / _bwd (include/bmc_hip_ssim.h
states the definition and every summation order).  Nothing here imports the code under test.

Two evaluations of the same definition:
  restatement   plain numpy in the KERNELS' order -- row sums left to right, the seven rows top to bottom; S added per lane down
                its strip of the tile, the 64 lanes in the tree l += l + o (o = 32 .. 1), the four waves ((w0 + w1) + w2) + w3,
                the tile partials in index order; the coefficients gathered row sums first (left to right), then top to bottom;
  conv2d        torch float64, the window means through F.conv2d with a uniform 7x7 kernel, the gradient through autograd.
The distance between the two on an input is float64's own sensitivity to summation order there: the GPU tests build their bars
on it (d for the loss, d_g for the gradient), so no constant is fixed in advance."""
import numpy as np
import torch
import torch.nn.functional as F

WIN, AP = 7, 6
K1, K2 = 0.01, 0.03


def _row_sums(t):
    """t [..., h, w] -> [..., h, w - 6]: the seven terms left to right."""
    pw = t.shape[-1] - AP
    s = t[..., 0:pw].copy()
    for k in range(1, WIN):
        s = s + t[..., k:k + pw]
    return s


def _col_sums(t):
    """t [..., h, w] -> [..., h - 6, w]: the seven rows top to bottom."""
    ph = t.shape[-2] - AP
    s = t[..., 0:ph, :].copy()
    for k in range(1, WIN):
        s = s + t[..., k:k + ph, :]
    return s


def terms(x, y, R):
    """x, y [P, h, w] float64 -> dict of the per-position maps [P, h - 6, w - 6] of the header, and the constants."""
    np_, nm1 = float(WIN * WIN), float(WIN * WIN - 1)
    C1, C2 = (K1 * R) * (K1 * R), (K2 * R) * (K2 * R)
    sx, sy, sxx, syy, sxy = (_col_sums(_row_sums(t)) for t in (x, y, x * x, y * y, x * y))
    with np.errstate(all="ignore"):
        ux, uy = sx / np_, sy / np_
        vx, vy, vxy = (sxx - sx * sx / np_) / nm1, (syy - sy * sy / np_) / nm1, (sxy - sx * sy / np_) / nm1
        A1, A2 = 2.0 * ux * uy + C1, 2.0 * vxy + C2
        B1, B2 = ux * ux + uy * uy + C1, vx + vy + C2
        D = B1 * B2
        S = (A1 * A2) / D
    return dict(ux=ux, uy=uy, A1=A1, A2=A2, B1=B1, B2=B2, D=D, S=S)


def _planes(x, y):
    x, y = np.asarray(x), np.asarray(y)
    assert x.ndim == 4 and x.shape == y.shape and min(x.shape[-2:]) >= WIN, (x.shape, y.shape)
    return x.astype(np.float64).reshape(-1, *x.shape[-2:]), y.astype(np.float64).reshape(-1, *x.shape[-2:])


def tile_partials(S, TH, TW):
    """S [P, ph, pw] -> [P, ntiles] in the tile launch's order (workgroups of 4 waves x 64 lanes, strips of TH / 4 rows)."""
    assert TW == 64 and TH % 4 == 0
    P, ph, pw = S.shape
    ty, tx = -(-ph // TH), -(-pw // TW)
    pad = np.zeros((P, ty * TH, tx * TW))
    pad[:, :ph, :pw] = S                                   # positions outside the image add exact zeros
    t = pad.reshape(P, ty, 4, TH // 4, tx, TW)             # [plane, tile row, wave, row of the strip, tile column, lane]
    acc = np.zeros((P, ty, 4, tx, TW))
    for r in range(TH // 4):                               # a lane: its column, top to bottom
        acc = acc + t[:, :, :, r]
    for o in (32, 16, 8, 4, 2, 1):                         # the lanes: l += l + o
        acc = acc[..., :o] + acc[..., o:2 * o]
    w = acc[..., 0]                                        # [P, ty, wave, tx]
    part = ((w[:, :, 0] + w[:, :, 1]) + w[:, :, 2]) + w[:, :, 3]
    return part.reshape(P, ty * tx)


def loss(x, y, R, TH=32, TW=64):
    """x, y [B, C, h, w] -> the loss as a Python float (float64, not yet rounded to float32), in the kernels' order."""
    xs, ys = _planes(x, y)
    S = terms(xs, ys, float(R))["S"]
    total = 0.0
    for v in tile_partials(S, TH, TW).reshape(-1).tolist():      # the finish: index order
        total += v
    return 1.0 - total / float(S.size)


def coefficients(x, y, R):
    """-> (alpha, beta, gamma), each [P, h - 6, w - 6] float64."""
    xs, ys = _planes(x, y)
    t = terms(xs, ys, float(R))
    np_ = float(WIN * WIN)
    cn = np_ / float(WIN * WIN - 1)
    k = (2.0 * cn) / np_
    with np.errstate(all="ignore"):
        gamma = -(k * t["S"]) / t["B2"]
        beta = (k * (t["A1"] / t["B1"])) / t["B2"]
        alpha = (((2.0 * t["uy"]) / t["B1"]) * (t["A2"] / t["B2"]) - (2.0 * t["ux"] * t["S"]) / t["B1"]) / np_ - beta * t["uy"] - gamma * t["ux"]
    return alpha, beta, gamma


def grad(x, y, R, gloss=1.0):
    """-> gloss * dloss/dx [B, C, h, w] float64 (not yet rounded to float32), in the backward kernel's order."""
    xs, ys = _planes(x, y)
    count = float(xs.shape[0] * (xs.shape[1] - AP) * (xs.shape[2] - AP))
    box = lambda c: _col_sums(_row_sums(np.pad(c, ((0, 0), (AP, AP), (AP, AP)))))      # positions outside the image: exact zeros
    sa, sb, sg = (box(c) for c in coefficients(x, y, R))
    g = (sa + ys * sb) + xs * sg
    return (-(g / count) * float(gloss)).reshape(np.asarray(x).shape)


# ------------------------------------------------------------------ the conv2d formulation, with autograd
def loss_conv2d(x, y, R):
    """x, y float64 torch tensors [B, C, h, w] -> the loss as a float64 tensor (differentiable in x)."""
    n = WIN * WIN
    cn = n / (n - 1.0)
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    k = torch.ones(1, 1, WIN, WIN, dtype=torch.float64) / n
    f = lambda t: F.conv2d(t.reshape(-1, 1, *t.shape[-2:]), k)
    ux, uy = f(x), f(y)
    vx, vy, vxy = cn * (f(x * x) - ux * ux), cn * (f(y * y) - uy * uy), cn * (f(x * y) - ux * uy)
    S = (2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return 1 - S.mean()


def conv2d_loss_and_grad(x, y, R):
    """numpy / torch float32 or float64 inputs -> (loss float, dloss/dx float64 numpy) of the conv2d formulation."""
    xt = torch.as_tensor(np.asarray(x)).to(torch.float64).requires_grad_()
    yt = torch.as_tensor(np.asarray(y)).to(torch.float64)
    L = loss_conv2d(xt, yt, float(R))
    (g,) = torch.autograd.grad(L, xt)
    return float(L.detach()), g.numpy()


# ------------------------------------------------------------------ inputs
def make_pair(B, C, h, w, seed):
    """Count-like images, float32 numpy [B, C, h, w]: gt = Poisson counts that are mostly zero, a region that is empty in both
    images, a few pixels at 255; pred = gt + noise (negative values included) outside the empty region."""
    r = np.random.default_rng(seed)
    gt = (r.poisson(0.3, (B, C, h, w)) * (r.random((B, C, h, w)) < 0.5)).astype(np.float32)
    for _ in range(3):
        gt[r.integers(B), r.integers(C), r.integers(h), r.integers(w)] = 255.0
    pred = (gt + 0.5 * r.standard_normal(gt.shape)).astype(np.float32)
    eh, ew = max(1, h // 2), max(1, w // 2)                # the top-left quarter: no event and no prediction
    if h >= 13 and w >= 9:
        gt[:, :, :eh, :ew] = 0.0
        pred[:, :, :eh, :ew] = 0.0
    return pred, gt


def shapes(TH, TW, PH, PW):
    """(h, w) of the kernel tests for forward tiles of TH x TW positions and backward tiles of PH x PW pixels: one position; one
    ragged row / column; every pixel's window set clipped at a border; ragged forward tiles in both directions; the backward apron
    crossing tile edges and clipped by the image."""
    return [(7, 7), (7, 8), (8, 7), (13, 9), (TH + 6 + 1, 2 * TW + 6 + 3), (2 * PH + 1, PW + 5)]
