"""Plain float64 restatement of bmc_head_loss_fwd / _bwd (include/bmc_hip_losses.h), written from the header's contract on top of
tests/head_resize_ref.py: torch float64 on the CPU, no tiling, no fixed summation order.

  pred = pixel_shuffle(xo, r) + bilinear(base)
  d    = pred - gt                          where the ground truth has the prediction's size (no resampling)
       = bicubic(pred -> gh x gw) - gt      otherwise
  loss = mean(rho(d))
  dlr  = pixel_unshuffle(dpred + (gloss / numel(gt)) R^T rho'(d)),   R^T the identity at equal sizes

  kind         rho(d)                                                  rho'(d)
  "l1"         |d|                                                     sign(d), sign(0) = 0
  "huber"      0.5 d^2 if |d| < delta else delta (|d| - 0.5 delta)     d if |d| < delta else delta sign(d)
  "charbonnier" sqrt(d^2 + eps^2)                                      d / sqrt(d^2 + eps^2)

rho and rho' are written out here, not taken from torch's losses: tests/test_head_loss_cpu.py ties them to F.l1_loss,
F.huber_loss, a hand-written Charbonnier and torch's float64 autograd; tests/test_gpu_head_loss.py holds the kernels to them."""
import torch

import head_resize_ref as HR
import streaming_ref as R

F64 = torch.float64
_d = R._d
KINDS = ("l1", "huber", "charbonnier")


def rho(kind, d, param):
    d = _d(d)
    a = d.abs()
    if kind == "l1":
        return a
    if kind == "huber":
        return torch.where(a < param, 0.5 * d * d, param * (a - 0.5 * param))
    if kind == "charbonnier":
        return torch.sqrt(d * d + param * param)
    raise ValueError(kind)


def drho(kind, d, param):
    d = _d(d)
    sgn = (d > 0).to(F64) - (d < 0).to(F64)
    if kind == "l1":
        return sgn
    if kind == "huber":
        return torch.where(d.abs() < param, d, param * sgn)
    if kind == "charbonnier":
        return d / torch.sqrt(d * d + param * param)
    raise ValueError(kind)


def fwd(xo, base, gt, r, kind, param):
    """xo [B,H,W,C r r], base [B,C,H,W], gt [B,C,gh,gw] -> (pred [B,C,rH,rW], d [B,C,gh,gw], loss), float64."""
    pred = R.shuffle_to_hr(xo, r, 1, base)
    gt = _d(gt)
    if tuple(gt.shape[-2:]) == tuple(pred.shape[-2:]):
        d = pred - gt
    else:
        d = HR.resize(pred, gt.shape[-2], gt.shape[-1]) - gt
    return pred, d, rho(kind, d, param).mean()


def bwd(dpred, d, gloss, r, HH, WW, kind, param, gather=False):
    """dlr [B,H,W,C r r] (float64) from d [B,C,gh,gw] (at equal sizes: pred - gt); dpred / gloss None = that gradient is
    absent (d is then not read)."""
    g = None
    if gloss is not None:
        d = _d(d)
        g = drho(kind, d, param)
        if tuple(d.shape[-2:]) != (HH, WW):
            g = HR.resize_t_gather(g, HH, WW) if gather else HR.resize_t(g, HH, WW)
        g = (float(_d(gloss)) / d.numel()) * g
    if dpred is not None:
        g = _d(dpred) if g is None else _d(dpred) + g
    return R.unshuffle_to_nhwc(g, r, 1)
