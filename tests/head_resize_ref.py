"""Plain float64 restatement of bmc_head_resize_mse_fwd / _bwd (include/bmc_hip.h), written from the header's contract on top of
tests/streaming_ref.py: torch float64 on the CPU, no tiling, no fixed summation order.

  pred = pixel_shuffle(xo, r) + bilinear(base)                        (streaming_ref.shuffle_to_hr)
  diff = bicubic(pred -> gh x gw) - gt,  loss = mean(diff^2)          (streaming_ref.bicubic_axis_matrix, axis by axis)
  dlr  = pixel_unshuffle(dpred + (2 gloss / numel(gt)) R^T diff)

R^T comes in two forms: `gather=True` is the one the kernel's contract states -- every prediction pixel sums the ground-truth
pixels whose clamped taps touch it, found from the taps themselves, not from a matrix -- and `gather=False` applies the
transposed axis matrices.  tests/test_head_resize_cpu.py checks both against the dense matrix and everything here against
torch's own float64 autograd; tests/test_gpu_head_resize.py checks the kernels against these functions."""
import math

import torch

import streaming_ref as R

F64 = torch.float64
_d = R._d


def _axis_touch(n_in, n_out):
    """touch[i] = [(dst, weight), ...]: the output indices whose taps read input index i along one axis, with the weight
    summed over the taps that the clamp folds onto i (float64; ATen's A = -0.75, src = (n_in/n_out)(dst + 0.5) - 0.5)."""
    A = -0.75
    scale = n_in / n_out
    inner = lambda v: ((A + 2.0) * v - (A + 3.0)) * v * v + 1.0
    outer = lambda v: ((A * v - 5.0 * A) * v + 8.0 * A) * v - 4.0 * A
    touch = [dict() for _ in range(n_in)]
    for dst in range(n_out):
        src = scale * (dst + 0.5) - 0.5
        i0 = math.floor(src)
        t = src - i0
        for k, w in enumerate((outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t))):
            i = min(max(i0 - 1 + k, 0), n_in - 1)
            touch[i][dst] = touch[i].get(dst, 0.0) + w
    return [sorted(d.items()) for d in touch]


def resize_t_gather(g, HH, WW):
    """g [..., gh, gw] -> [..., HH, WW]: the transposed bicubic resize as a gather, rows of g first, then its columns."""
    g = _d(g)
    gh, gw = g.shape[-2:]
    tx, ty = _axis_touch(WW, gw), _axis_touch(HH, gh)
    tmp = torch.zeros(g.shape[:-1] + (WW,), dtype=F64)
    for x, lst in enumerate(tx):
        for X, w in lst:
            tmp[..., x] += w * g[..., X]
    out = torch.zeros(g.shape[:-2] + (HH, WW), dtype=F64)
    for y, lst in enumerate(ty):
        for Y, w in lst:
            out[..., y, :] += w * tmp[..., Y, :]
    return out


def resize(pred, gh, gw):
    """pred [..., HH, WW] -> [..., gh, gw]: the bicubic operator axis by axis."""
    pred = _d(pred)
    HH, WW = pred.shape[-2:]
    return R.bicubic_axis_matrix(HH, gh) @ pred @ R.bicubic_axis_matrix(WW, gw).T


def resize_t(g, HH, WW):
    g = _d(g)
    gh, gw = g.shape[-2:]
    return R.bicubic_axis_matrix(HH, gh).T @ g @ R.bicubic_axis_matrix(WW, gw)


def fwd(xo, base, gt, r):
    """xo [B,H,W,C r r], base [B,C,H,W], gt [B,C,gh,gw] -> (pred [B,C,rH,rW], diff [B,C,gh,gw], loss), float64."""
    pred = R.shuffle_to_hr(xo, r, 1, base)
    gt = _d(gt)
    diff = resize(pred, gt.shape[-2], gt.shape[-1]) - gt
    return pred, diff, (diff ** 2).mean()


def bwd(dpred, diff, gloss, r, HH, WW, gather=False):
    """dlr [B,H,W,C r r] (float64); dpred / gloss None = that gradient is absent (diff is then not read)."""
    g = None
    if gloss is not None:
        diff = _d(diff)
        rt = resize_t_gather(diff, HH, WW) if gather else resize_t(diff, HH, WW)
        g = (2.0 * float(_d(gloss)) / diff.numel()) * rt
    if dpred is not None:
        g = _d(dpred) if g is None else _d(dpred) + g
    return R.unshuffle_to_nhwc(g, r, 1)
