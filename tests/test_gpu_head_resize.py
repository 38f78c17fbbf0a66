"""bmc_head_resize_mse_fwd / _bwd (csrc/head_resize.hip) alone against their float64 restatement (tests/head_resize_ref.py), and
the training / validation step that now takes them whenever the ground truth is not of the prediction's size.

Kernel tests: through ctypes into guarded buffers, with the rules of tests/test_gpu_streaming_kernels.py -- bit-exact where the
contract says so (pred == ops.head, dlr of a dpred alone == the unshuffle, run-to-run determinism, wrapper == direct calls), the
4x rule (vs_aten) elsewhere: the kernel's largest elementwise error against float64 is at most 4x the larger of the error of
ATen's fp32 composition on the CPU (pixel_shuffle + bilinear + bicubic interpolate + mse_loss and its autograd) and one ulp.
The backward is handed ATen's own fp32 diff, so kernel, ATen and float64 transpose the same tensor.

Launch arithmetic the shapes come from (csrc/head_resize.hip): 256 threads, blocks = max(ceil(npred / 1024), ceil(ngt / 256))
capped at 2048, two grid-stride loops (prediction elements, then ground-truth elements); the backward ceil(npred / 256) blocks
(ceil(npred / 1024) without gloss), capped at 2048.  The last case is above one pass of the capped grid on both sides.

Measured on an MI355X (pytest -s, the RATIO lines), 54 comparisons: per group their number, the largest ratio and its case.  The
bound is 4; no case reaches 2.

RATIO_TABLE_BEGIN
group                             cases  max ratio  at
head_resize_fwd diff                 14       1.19  r=4 C=2 B=2 3x5->5x7 gt=strided
head_resize_fwd loss                 14       1.94  r=4 C=2 B=2 3x5->5x7 gt=contiguous  (kernel 9.2e-07 = 1.9 ulp, ATen 3.0e-08)
head_resize_bwd gloss border          7       1.11  r=4 C=2 B=2 3x5->13x22
head_resize_bwd gloss interior        6       1.10  r=4 C=2 B=2 3x5->12x18
head_resize_bwd both border           7       0.50  r=4 C=2 B=2 31x56->124x222
head_resize_bwd both interior         6       0.50  r=4 C=2 B=2 31x56->124x222
RATIO_TABLE_END
(1x1 -> 3x1 has no interior: its four prediction pixels are all border.)

Plain model, fused against unfused (test_plain_model_fused_equals_unfused): the losses agree to all printed digits (1.79646540),
the 24 gradients differ by rel-L2 7.7e-08 .. 2.7e-07 against the bar of 1e-4.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import head_resize_ref as HR
import streaming_ref as R
from test_gpu_r2 import _gpu, _restore_math_mode, load, rel_l2  # noqa: F401
from test_gpu_streaming_kernels import SENT, Guarded, _base, _edges, call, refused, vs_aten

pytestmark = pytest.mark.gpu

# r, C, H, W (LR), gh, gw, B
CASES = [
    (2, 1, 1, 1, 3, 1, 2),             # every tap clamped, up in y and down in x
    (4, 2, 3, 5, 12, 18, 2),           # x only
    (4, 2, 3, 5, 11, 20, 2),           # y only
    (4, 2, 3, 5, 13, 22, 2),           # up on both axes
    (4, 2, 3, 5, 5, 7, 2),             # strong reduction: many taps per prediction pixel in the backward
    (4, 2, 31, 56, 124, 222, 2),       # EventZoom itself; the y axis is an exact identity
    (2, 2, 363, 363, 724, 730, 1),     # 1 054 152 prediction and 1 057 040 ground-truth elements > 2048 * 256 threads
]
LAYOUTS = ["contiguous", "strided"]


def _name(case):
    r, C, H, W, gh, gw, B = case
    return "r=%d C=%d B=%d %dx%d->%dx%d" % (r, C, B, H, W, gh, gw)


def _aten(xo, base, gt, r):
    pred = (F.pixel_shuffle(xo.permute(0, 3, 1, 2), r)
            + F.interpolate(base, scale_factor=r, mode="bilinear", align_corners=False)).contiguous()
    sp = F.interpolate(pred, size=gt.shape[-2:], mode="bicubic", align_corners=False)
    return pred, sp


@functools.lru_cache(maxsize=None)
def _case(case, layout):
    """Operands on the GPU, ATen's fp32 composition and the float64 reference on the CPU: built once, shared, never written."""
    r, C, H, W, gh, gw, B = case
    dev = _gpu()
    torch.manual_seed(r * 1000 + C * 100 + H + gh + 2)
    xo = torch.randn(B, H, W, C * r * r, device=dev)
    base = _base(B, C, H, W, "slice" if layout == "strided" else "contiguous", dev)
    if layout == "contiguous":
        gt = torch.randn(B, C, gh, gw, device=dev)
    else:                                                            # batch stride larger than C*gh*gw
        gt = torch.randn(B, C + 1, gh, gw, device=dev)[:, :C]
        assert gt.stride(0) > C * gh * gw
    xc, bc, gc = xo.cpu(), base.cpu().contiguous(), gt.cpu().contiguous()
    apred, asp = _aten(xc, bc, gc, r)
    rpred, rdiff, rloss = HR.fwd(xc, bc, gc, r)
    return dict(xo=xo, base=base, gt=gt, gtc=gc, apred=apred, adiff=asp - gc, aloss=F.mse_loss(asp, gc), rpred=rpred,
                rdiff=rdiff, rloss=rloss)


def _fwd_args(case, k, pred, diff, partials, loss):
    r, C, H, W, gh, gw, B = case
    return (k["xo"].data_ptr(), B, C, H, W, r, k["base"].data_ptr(), *k["base"].stride(), k["gt"].data_ptr(), k["gt"].stride(0),
            gh, gw, pred.ptr(), diff.ptr() if diff is not None else None, partials.ptr(), loss.ptr())


def _bwd_call(case, dpred, diff, gloss, dlr):
    r, C, H, W, gh, gw, B = case
    p = lambda t: t.data_ptr() if t is not None else None
    call("_head_resize_mse_bwd", "bmc_head_resize_mse_bwd", p(dpred), p(diff), p(gloss), B, C, H, W, r, gh, gw, dlr.ptr())


# ================================================================== forward
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=_name)
def test_head_resize_mse_fwd_vs_float64(case, layout):
    dev = _gpu()
    from bmc_hip import ops
    r, C, H, W, gh, gw, B = case
    k = _case(case, layout)
    npred, ngt = B * C * H * r * W * r, B * C * gh * gw
    pred, diff, partials, loss = Guarded(npred, dev), Guarded(ngt, dev), Guarded(2048, dev), Guarded(1, dev)
    call("_head_resize_mse_fwd", "bmc_head_resize_mse_fwd", *_fwd_args(case, k, pred, diff, partials, loss))
    gp, gd, gl = pred.cpu((B, C, H * r, W * r)), diff.cpu((B, C, gh, gw)), loss.cpu()
    used = int((partials.cpu() != SENT).sum())
    assert used == min(max(-(-npred // 1024), -(-ngt // 256)), 2048)
    # the prediction recurs into the next window: the bits ops.head gives, whichever loss path ran
    assert torch.equal(gp, ops.head(k["xo"], k["base"], r).cpu())
    name = "head_resize_fwd %s gt=%s" % (_name(case), layout)
    vs_aten(name + " diff", gd, k["adiff"], k["rdiff"])
    vs_aten(name + " loss", gl, k["aloss"].reshape(1), k["rloss"].reshape(1))
    # run-to-run identical
    pred2, diff2, loss2 = Guarded(npred, dev), Guarded(ngt, dev), Guarded(1, dev)
    call("_head_resize_mse_fwd", "bmc_head_resize_mse_fwd", *_fwd_args(case, k, pred2, diff2, partials, loss2))
    assert torch.equal(diff2.cpu((B, C, gh, gw)), gd) and torch.equal(loss2.cpu(), gl) and torch.equal(pred2.cpu(), gp.reshape(-1))
    # forward only: diff = NULL stores nothing and changes no bit of pred or loss
    pred3, diff3, loss3 = Guarded(npred, dev), Guarded(ngt, dev), Guarded(1, dev)
    call("_head_resize_mse_fwd", "bmc_head_resize_mse_fwd", *_fwd_args(case, k, pred3, None, partials, loss3))
    assert diff3.untouched()
    assert torch.equal(pred3.cpu(), gp.reshape(-1)) and torch.equal(loss3.cpu(), gl)
    # the wrapper launches the same kernels: forward only under no_grad, with diff saved when a backward can follow
    with torch.no_grad():
        wp, wl = ops.head_resize_mse(k["xo"], k["base"], k["gt"], r)
    assert torch.equal(wp.cpu(), gp) and torch.equal(wl.cpu().reshape(1), gl)
    xo = k["xo"].clone().requires_grad_()
    wp, wl = ops.head_resize_mse(xo, k["base"], k["gt"], r)
    assert torch.equal(wp.cpu(), gp) and torch.equal(wl.cpu().reshape(1), gl)
    torch.manual_seed(gh * 7 + r)
    dpred, gloss = torch.randn(B, C, H * r, W * r, device=dev), torch.tensor(0.37, device=dev)
    torch.autograd.backward([wp, wl], [dpred, gloss])
    dlr = Guarded(npred, dev)
    _bwd_call(case, dpred, diff.t, gloss, dlr)
    assert torch.equal(xo.grad.cpu(), dlr.cpu((B, H, W, C * r * r)))


# ================================================================== backward
@pytest.mark.parametrize("which", ["dpred", "gloss", "both"])
@pytest.mark.parametrize("case", CASES, ids=_name)
def test_head_resize_mse_bwd_vs_float64(case, which):
    dev = _gpu()
    r, C, H, W, gh, gw, B = case
    k = _case(case, "contiguous")
    HH, WW = H * r, W * r
    torch.manual_seed(H * 7 + r + gw)
    dpredc = torch.randn(B, C, HH, WW) if which != "gloss" else None
    glossc = torch.tensor(0.37) if which != "dpred" else None
    diffc = k["adiff"]                                               # the same fp32 diff goes to the kernel, ATen and float64
    dpred = dpredc.to(dev) if dpredc is not None else None
    gloss = glossc.to(dev) if glossc is not None else None
    diff = diffc.to(dev)
    dlr = Guarded(B * C * HH * WW, dev)
    _bwd_call(case, dpred, diff if which != "dpred" else None, gloss, dlr)
    got = dlr.cpu((B, H, W, C * r * r))
    if which == "dpred":
        assert torch.equal(got, R.unshuffle_to_nhwc(dpredc, r, 1))   # a pure permutation; diff is not read (NULL here)
        return
    leaf = k["apred"].clone().requires_grad_()                       # ATen: autograd through the fp32 composition
    sp = F.interpolate(leaf, size=(gh, gw), mode="bicubic", align_corners=False)
    assert torch.equal((sp - k["gtc"]).detach(), diffc)
    (g,) = torch.autograd.grad(F.mse_loss(sp, k["gtc"]), leaf, glossc)
    if dpredc is not None:
        g = dpredc + g
    ref = R.shuffle_to_hr(HR.bwd(dpredc, diffc, glossc, r, HH, WW), r)       # back in the prediction's layout (a permutation)
    gotp = R.shuffle_to_hr(got, r)
    e = _edges(gotp.shape)
    name = "head_resize_bwd %s %s" % (_name(case), which)
    vs_aten(name + " border", gotp, g, ref, e)
    vs_aten(name + " interior", gotp, g, ref, ~e)
    dlr2 = Guarded(B * C * HH * WW, dev)                             # run-to-run identical
    _bwd_call(case, dpred, diff, gloss, dlr2)
    assert torch.equal(dlr2.cpu((B, H, W, C * r * r)), got)


def test_head_resize_mse_refuses():
    dev = _gpu()
    a = torch.ones(64, device=dev)
    p = a.data_ptr()
    pred, diff, part, loss, dlr = Guarded(64, dev), Guarded(64, dev), Guarded(2048, dev), Guarded(1, dev), Guarded(64, dev)
    ok = [p, 1, 1, 2, 2, 2, p, 4, 4, 2, 1, p, 12, 3, 4, pred.ptr(), diff.ptr(), part.ptr(), loss.ptr()]
    for i in (0, 6, 11, 15, 17, 18):                                 # xo, base, gt, pred, partials, loss
        args = list(ok)
        args[i] = None
        refused("_head_resize_mse_fwd", "bmc_head_resize_mse_fwd", *args)
    args = list(ok)
    args[13] = 0                                                     # gh = 0
    refused("_head_resize_mse_fwd", "bmc_head_resize_mse_fwd", *args)
    refused("_head_resize_mse_bwd", "bmc_head_resize_mse_bwd", None, p, None, 1, 1, 2, 2, 2, 3, 4, dlr.ptr())    # no gradient
    refused("_head_resize_mse_bwd", "bmc_head_resize_mse_bwd", p, None, p, 1, 1, 2, 2, 2, 3, 4, dlr.ptr())       # gloss without diff
    refused("_head_resize_mse_bwd", "bmc_head_resize_mse_bwd", p, p, p, 1, 1, 2, 2, 2, 3, 4, None)               # no dlr
    refused("_head_resize_mse_bwd", "bmc_head_resize_mse_bwd", p, p, p, 1, 1, 2, 2, 2, 0, 4, dlr.ptr())          # gh = 0
    assert all(g.untouched() for g in (pred, diff, part, loss, dlr))


# ================================================================== the model and the steps
def _raise(what):
    def f(*a, **k):
        raise AssertionError(what + " was called: the unfused chain ran")
    return f


def _golden_model(dev):
    from models.BMCNet import BMCNet
    from test_gpu_parity import _load_sd
    z = load("bmcnet_resize.npz")
    scale, n_c, n_b, B, H, W, nwin, gh, gw = (int(v) for v in z["meta"])
    m = BMCNet(scale, n_c, n_b)
    _load_sd(m, z)
    m.to(dev)
    return m, z, torch.tensor(z["frames"]).to(dev), torch.tensor(z["gts"]).to(dev), n_c, scale


@pytest.mark.parametrize("path", ["fused", "unfused"])
def test_bptt_step_golden_resize_branch(path, monkeypatch):
    """The reference's loop with the size-mismatch branch taken (golden bmcnet_resize.npz: 28x56 prediction, 28x54 ground truth):
    loss and every parameter gradient, at the bars of test_gpu_r2.test_bptt_with_resize_branch_golden, through the fused launches
    (the unfused chain's entry points raise) and, same weights, through the unfused chain selected by a loss_fn of the caller's."""
    dev = _gpu()
    from bmc_hip import lib, ops
    from test_gpu_parity import _check_grads
    from train_step import bptt_step
    m, z, frames, gts, n_c, scale = _golden_model(dev)
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    if path == "fused":
        monkeypatch.setattr(lib, "_bicubic_fwd", _raise("bmc_bicubic_resize_fwd"))
        monkeypatch.setattr(ops, "head", _raise("ops.head"))
        loss, _ = bptt_step(m, opt, frames, gts, n_c, scale)
    else:
        monkeypatch.setattr(ops, "head_resize_mse", _raise("ops.head_resize_mse"))
        loss, _ = bptt_step(m, opt, frames, gts, n_c, scale, loss_fn=lambda a, b: F.mse_loss(a, b))
    assert abs(loss.item() - float(z["loss"])) < 1e-4 * abs(float(z["loss"]))
    assert _check_grads(m, z, 1e-3) >= 40


def _plain_case(dev):
    from models.BMCNet_plain import BMCNet_plain
    torch.manual_seed(11)
    scale, n_c, B, H, W, L = 4, 16, 2, 6, 9, 4                      # 3 windows; prediction 24x36, ground truth 22x35
    m = BMCNet_plain(scale, n_c, 1)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(5.0).add_(0.02 * torch.randn_like(p))
    inp = torch.poisson(torch.full((B, L, 2, H, W), 0.3)).to(dev)
    gt = torch.poisson(torch.full((B, L, 2, 22, 35), 0.3)).to(dev)
    return m.to(dev), inp, gt, n_c, scale


def _step(m, inp, gt, n_c, scale, **kw):
    from train_step import bptt_step
    m = copy.deepcopy(m)
    loss, mse = bptt_step(m, torch.optim.SGD(m.parameters(), lr=0.0), inp, gt, n_c, scale, plain=True, **kw)
    return loss, mse, {k: p.grad.clone() for k, p in m.named_parameters()}


def test_plain_model_fused_equals_unfused():
    """BMCNet_plain, LR 6x9 -> ground truth 22x35, 3 windows: the two paths differ only in summation order inside one tiny
    operator (and in where 2 gloss / numel is multiplied in): loss within 1e-5 relative, every gradient within rel-L2 1e-4."""
    dev = _gpu()
    m, inp, gt, n_c, scale = _plain_case(dev)
    lf, _, gf = _step(m, inp, gt, n_c, scale)
    lu, _, gu = _step(m, inp, gt, n_c, scale, loss_fn=lambda a, b: F.mse_loss(a, b))
    print("plain fused %.8f unfused %.8f" % (lf.item(), lu.item()))
    assert abs(lf.item() - lu.item()) <= 1e-5 * abs(lu.item())
    assert len(gf) == len(gu) > 0
    for k in gu:
        d = rel_l2(gf[k], gu[k])
        print("plain grad %-40s rel-L2 %.3e" % (k, d))
        assert d <= 1e-4, (k, d)


def test_recompute_is_bit_identical_at_a_mismatched_size():
    dev = _gpu()
    m, inp, gt, n_c, scale = _plain_case(dev)
    l0, m0, g0 = _step(m, inp, gt, n_c, scale)
    l1, m1, g1 = _step(m, inp, gt, n_c, scale, recompute=True)
    assert torch.equal(l0, l1) and torch.equal(m0, m1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_valid_step_golden_forward_only(monkeypatch):
    dev = _gpu()
    from bmc_hip import lib, ops
    from train_step import valid_step
    m, z, frames, gts, n_c, scale = _golden_model(dev)
    diffs = []
    real = lib._head_resize_mse_fwd

    def spy(*args):
        diffs.append(args[16])
        return real(*args)

    monkeypatch.setattr(lib, "_head_resize_mse_fwd", spy)
    monkeypatch.setattr(lib, "_bicubic_fwd", _raise("bmc_bicubic_resize_fwd"))
    monkeypatch.setattr(ops, "head", _raise("ops.head"))
    for mode in (True, False):
        m.train(mode)
        loss, mse = valid_step(m, frames, gts, n_c, scale)
        assert m.training is mode
        assert abs(loss.item() - float(z["loss"])) < 1e-4 * abs(float(z["loss"]))
        assert not loss.requires_grad and not mse.requires_grad
    assert all(p.grad is None for p in m.parameters())
    nwin = int(z["meta"][6])
    assert len(diffs) == 2 * nwin and all(d is None for d in diffs)    # nothing of the ground truth's size is stored


def test_same_size_ground_truth_still_takes_head_mse(monkeypatch):
    """forward_loss with a ground truth of the prediction's size: ops.head_mse's outputs, unchanged in any bit."""
    dev = _gpu()
    from bmc_hip import ops
    m, inp, _, n_c, scale = _plain_case(dev)
    B, _, _, H, W = inp.shape
    gt = torch.poisson(torch.full((B, 2, scale * H, scale * W), 0.3)).to(dev)
    seen = []
    real = ops.head_mse

    def spy(xo, base, g, r):
        out = real(xo, base, g, r)
        seen.append((xo.detach(), base, out))
        return out

    monkeypatch.setattr(ops, "head_mse", spy)
    monkeypatch.setattr(ops, "head_resize_mse", _raise("ops.head_resize_mse"))
    z = lambda c: torch.zeros(B, c, H, W, device=dev)
    x = inp[:, 0:2].transpose(1, 2)
    with torch.no_grad():
        h, pred, mse = m.forward_loss(x, z(n_c), z(2 * scale * scale), True, gt)
        h2, pred2 = m(x, z(n_c), z(2 * scale * scale), True)
    assert len(seen) == 1
    xo, base, (p0, l0) = seen[0]
    assert torch.equal(pred, p0) and torch.equal(mse, l0)
    monkeypatch.undo()
    p1, l1 = ops.head_mse(xo, base, gt, scale)
    assert torch.equal(pred, p1) and torch.equal(mse, l1) and torch.equal(pred, pred2) and torch.equal(h, h2)
