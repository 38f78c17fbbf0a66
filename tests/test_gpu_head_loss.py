"""bmc_head_loss_fwd / _bwd (include/bmc_hip_losses.h, csrc/head_resize.hip: the head with an L1, Huber or Charbonnier loss, ground truth of either size)
alone against their float64 restatement (tests/head_loss_ref.py), and the training / validation step that takes them when
loss_fn is a bmc_hip.losses object.

Kernel tests: through ctypes into guarded buffers, with the rules of tests/test_gpu_streaming_kernels.py -- bit-exact where the
contract says so (pred == ops.head, dlr of a dpred alone == the unshuffle, run-to-run determinism, wrapper == direct calls, the
forward-only form writes nothing of the ground truth's size), the 4x rule (vs_aten) elsewhere: the kernel's largest elementwise
error against float64 is at most 4x the larger of the error of ATen's fp32 composition on the CPU (pixel_shuffle + bilinear +
bicubic interpolate + F.l1_loss / F.huber_loss / a hand-written Charbonnier, and their autograd) and one ulp.

Forward operands are random normal: d passes through 0 and +-delta only by rounding, and rho is continuous there.  The backward
is handed its saved input directly, and rho' is NOT continuous at 0 (L1) -- so that input is dyadic: d is a multiple of 1/64 that
is never 0 or +-delta (so at least 1/64 from either kink: no fp32 rounding crosses one, no element is excluded), except for a
handful of entries placed at exactly 0 and exactly +-delta, which pin sign(0) = 0 and the Huber boundary (both branches give
+-delta there).  At the prediction's own size the kernel reads pred and gt: gt holds integer counts and pred = d + gt, exact in
fp32, so pred - gt is that d bit for bit.

Launch arithmetic (csrc/head_resize.hip): 256 threads; forward blocks = ceil(npred / 1024), and where the sizes differ the larger
of that and ceil(ngt / 256), capped at 2048; backward ceil(npred / 256) blocks where it gathers (gloss and sizes differ),
ceil(npred / 1024) otherwise, capped at 2048.  The 363x363 case is above one pass of the capped grid on both sides.

Measured on an MI355X (pytest -s, the RATIO lines): per group the number of comparisons, the largest ratio and its case.  The
bound is 4.

RATIO_TABLE_BEGIN
group                                     cases  max ratio  at
fwd d (sizes differ)   l1                     8       1.38  r=2 C=1 B=2 1x1->3x1 gt=strided
fwd d                  huber                  8       1.38  (the same d: one kernel body, three pointwise functions)
fwd d                  charbonnier            8       1.38
fwd loss               l1                    12       0.71  r=4 C=2 B=2 3x5->12x20 gt=strided
fwd loss               huber                 12       1.90  r=4 C=2 B=2 3x5->13x22 gt=contiguous  (kernel 2.3e-07 = 1.9 ulp, ATen 1.1e-07)
fwd loss               charbonnier           12       1.00  r=4 C=2 B=2 3x5->13x22 gt=contiguous
bwd gloss border       l1 / huber / charb.    4       1.06 / 1.06 / 1.03  r=4 C=2 B=2 3x5->5x7
bwd gloss interior     l1 / huber / charb.    3       1.00 / 1.05 / 1.03  363x363->724x730, 3x5->13x22, 3x5->13x22
bwd both border        l1 / huber / charb.    4       0.50 / 0.50 / 0.50  r=2 C=2 B=1 363x363->724x730
bwd both interior      l1 / huber / charb.    3       0.50 / 0.50 / 0.49
bwd gloss, same size   l1 / huber / charb.    2       0.00 / 0.00 / 0.76  r=4 C=2 B=2 3x5->12x20 (L1 and Huber are exact there)
bwd both, same size    l1 / huber / charb.    2       0.45 / 0.49 / 0.49  r=4 C=2 B=2 3x5->12x20
RATIO_TABLE_END
114 comparisons; no case reaches 2.  (1x1 -> 3x1 has no interior: its four prediction pixels are all border.)

Model level (BMCNet_plain, LR 6x9, 3 windows, ground truth 22x35 and 24x36; BMCNet on the golden bmcnet_resize.npz with Huber),
fused against the unfused chain with the same loss object, bars 1e-5 (loss, relative) and 1e-4 (every gradient, rel-L2):
MODEL_TABLE_BEGIN
case                          fused loss    unfused loss  relative   gradients  worst rel-L2
plain l1          gt 22x35    1.71709561    1.71709561    0          24         2.6e-07
plain huber(0.5)  gt 22x35    0.57617688    0.57617688    0          24         2.9e-07
plain charbonnier gt 22x35    1.71711898    1.71711898    0          24         1.1e-06
plain l1          gt 24x36    1.81960511    1.81960511    0          24         0  (sign(pred - gt): the same bits both ways)
plain huber(0.5)  gt 24x36    0.62130523    0.62130523    0          24         2.3e-07
plain charbonnier gt 24x36    1.81962478    1.81962490    6.6e-08    24         1.7e-07
BMCNet huber(1.0) golden      0.61331201    0.61331201    0          52         3.6e-07
MODEL_TABLE_END
recompute=True reproduced the fused step bit for bit in all six plain cases.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import head_loss_ref as HL
import streaming_ref as R
from test_gpu_head_resize import _golden_model, _plain_case, _raise, _step
from test_gpu_r2 import _gpu, _restore_math_mode, rel_l2  # noqa: F401
from test_gpu_streaming_kernels import SENT, Guarded, _base, _edges, vs_aten

pytestmark = pytest.mark.gpu

# r, C, H, W (LR), gh, gw, B
RESIZE_CASES = [
    (2, 1, 1, 1, 3, 1, 2),             # every tap clamped
    (4, 2, 3, 5, 13, 22, 2),           # up on both axes
    (4, 2, 3, 5, 5, 7, 2),             # strong reduction: many taps per prediction pixel in the backward
    (2, 2, 363, 363, 724, 730, 1),     # more elements than 2048 * 256 threads: grid-stride loops, all 2048 partials
]
SAME_CASES = [
    (4, 2, 3, 5, 12, 20, 2),
    (2, 1, 1, 1, 2, 2, 1),
]
CASES = RESIZE_CASES + SAME_CASES
LAYOUTS = ["contiguous", "strided"]
DELTA, EPS = 1.0, 1e-3
KINDS = [("l1", 0.0), ("huber", DELTA), ("charbonnier", EPS)]


def call(fn_name, what, *args):
    """tests/test_gpu_streaming_kernels.call for the entry points of include/bmc_hip_losses.h (bound by bmc_hip/loss_lib.py)."""
    from bmc_hip import lib, loss_lib, ops
    lib.call(getattr(loss_lib, fn_name), what, *args, ops._stream())


def refused(fn_name, what, *args):
    with pytest.raises(RuntimeError, match=what):
        call(fn_name, what, *args)


def _kind_const(kind):
    from bmc_hip import loss_lib
    return loss_lib.const("BMC_LOSS_" + kind.upper())


def _loss_obj(kind, param):
    from bmc_hip import losses
    return {"l1": losses.L1, "huber": lambda: losses.Huber(param), "charbonnier": lambda: losses.Charbonnier(param)}[kind]()


def _aten_loss(kind, param, a, b):
    """ATen's fp32 composition of the loss (the hand-written Charbonnier is the usual sqrt(d^2 + eps^2))."""
    if kind == "l1":
        return F.l1_loss(a, b)
    if kind == "huber":
        return F.huber_loss(a, b, delta=param)
    return torch.sqrt((a - b) ** 2 + param ** 2).mean()


def _name(case):
    r, C, H, W, gh, gw, B = case
    return "r=%d C=%d B=%d %dx%d->%dx%d" % (r, C, B, H, W, gh, gw)


def _is_resize(case):
    r, C, H, W, gh, gw, B = case
    return (gh, gw) != (H * r, W * r)


@functools.lru_cache(maxsize=None)
def _case(case, layout):
    """Operands on the GPU, ATen's fp32 composition and the float64 reference on the CPU: built once per (case, layout), shared
    by the three kinds, never written."""
    r, C, H, W, gh, gw, B = case
    dev = _gpu()
    torch.manual_seed(r * 1000 + C * 100 + H + gh + 5)
    xo = torch.randn(B, H, W, C * r * r, device=dev)
    base = _base(B, C, H, W, "slice" if layout == "strided" else "contiguous", dev)
    if layout == "contiguous":
        gt = torch.randn(B, C, gh, gw, device=dev)
    else:                                                            # batch stride larger than C*gh*gw
        gt = torch.randn(B, C + 1, gh, gw, device=dev)[:, :C]
        assert gt.stride(0) > C * gh * gw
    xc, bc, gc = xo.cpu(), base.cpu().contiguous(), gt.cpu().contiguous()
    apred = (F.pixel_shuffle(xc.permute(0, 3, 1, 2), r)
             + F.interpolate(bc, scale_factor=r, mode="bilinear", align_corners=False)).contiguous()
    asp = F.interpolate(apred, size=(gh, gw), mode="bicubic", align_corners=False) if _is_resize(case) else apred
    rpred, rd, _ = HL.fwd(xc, bc, gc, r, "l1", 0.0)
    return dict(xo=xo, base=base, gt=gt, gtc=gc, asp=asp, ad=asp - gc, rpred=rpred, rd=rd)


def _fwd_args(case, k, pred, dsave, partials, loss, kind, param):
    r, C, H, W, gh, gw, B = case
    return (k["xo"].data_ptr(), B, C, H, W, r, k["base"].data_ptr(), *k["base"].stride(), k["gt"].data_ptr(), k["gt"].stride(0),
            gh, gw, pred.ptr(), dsave.ptr() if dsave is not None else None, partials.ptr(), loss.ptr(),
            _kind_const(kind), param)


def _bwd_call(case, dpred, dsave, pred, gt, gloss, kind, param, dlr):
    r, C, H, W, gh, gw, B = case
    p = lambda t: t.data_ptr() if t is not None else None
    call("_head_loss_bwd", "bmc_head_loss_bwd", p(dpred), p(dsave), p(pred), p(gt), gt.stride(0) if gt is not None else 0, p(gloss),
         B, C, H, W, r, gh, gw, _kind_const(kind), param, dlr.ptr())


# ================================================================== forward
@pytest.mark.parametrize("kind,param", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=_name)
def test_head_loss_fwd_vs_float64(case, layout, kind, param):
    dev = _gpu()
    from bmc_hip import ops
    r, C, H, W, gh, gw, B = case
    k = _case(case, layout)
    resize = _is_resize(case)
    npred, ngt = B * C * H * r * W * r, B * C * gh * gw
    pred, dsave, partials, loss = Guarded(npred, dev), Guarded(ngt, dev), Guarded(2048, dev), Guarded(1, dev)
    call("_head_loss_fwd", "bmc_head_loss_fwd", *_fwd_args(case, k, pred, dsave, partials, loss, kind, param))
    gp, gl = pred.cpu((B, C, H * r, W * r)), loss.cpu()
    used = int((partials.cpu() != SENT).sum())
    assert used == min(max(-(-npred // 1024), -(-ngt // 256) if resize else 1), 2048)
    # the prediction recurs into the next window: the bits ops.head gives, whichever loss ran
    assert torch.equal(gp, ops.head(k["xo"], k["base"], r).cpu())
    name = "head_loss_fwd %s %s gt=%s" % (kind, _name(case), layout)
    if resize:
        gd = dsave.cpu((B, C, gh, gw))
        vs_aten(name + " d", gd, k["ad"], k["rd"])
    else:
        assert dsave.untouched()                                     # nothing new is saved at the prediction's own size
    aloss = _aten_loss(kind, param, k["asp"], k["gtc"])
    rloss = HL.rho(kind, k["rd"], param).mean()
    vs_aten(name + " loss", gl, aloss.reshape(1), rloss.reshape(1))
    # run-to-run identical
    pred2, dsave2, loss2 = Guarded(npred, dev), Guarded(ngt, dev), Guarded(1, dev)
    call("_head_loss_fwd", "bmc_head_loss_fwd", *_fwd_args(case, k, pred2, dsave2, partials, loss2, kind, param))
    assert torch.equal(loss2.cpu(), gl) and torch.equal(pred2.cpu(), gp.reshape(-1))
    assert not resize or torch.equal(dsave2.cpu((B, C, gh, gw)), gd)
    # forward only: dsave = NULL stores nothing and changes no bit of pred or loss
    pred3, dsave3, loss3 = Guarded(npred, dev), Guarded(ngt, dev), Guarded(1, dev)
    call("_head_loss_fwd", "bmc_head_loss_fwd", *_fwd_args(case, k, pred3, None, partials, loss3, kind, param))
    assert dsave3.untouched()
    assert torch.equal(pred3.cpu(), gp.reshape(-1)) and torch.equal(loss3.cpu(), gl)
    # the wrapper launches the same kernels: forward only under no_grad, and with a backward that equals the direct call
    L = _loss_obj(kind, param)
    with torch.no_grad():
        wp, wl = ops.head_loss(k["xo"], k["base"], k["gt"], r, L)
    assert torch.equal(wp.cpu(), gp) and torch.equal(wl.cpu().reshape(1), gl)
    xo = k["xo"].clone().requires_grad_()
    wp, wl = ops.head_loss(xo, k["base"], k["gt"], r, L)
    assert torch.equal(wp.cpu(), gp) and torch.equal(wl.cpu().reshape(1), gl)
    torch.manual_seed(gh * 7 + r)
    dpred, gloss = torch.randn(B, C, H * r, W * r, device=dev), torch.tensor(0.37, device=dev)
    torch.autograd.backward([wp, wl], [dpred, gloss])
    dlr = Guarded(npred, dev)
    if resize:
        _bwd_call(case, dpred, dsave.t, None, None, gloss, kind, param, dlr)
    else:
        _bwd_call(case, dpred, None, pred.t, k["gt"], gloss, kind, param, dlr)
    assert torch.equal(xo.grad.cpu(), dlr.cpu((B, H, W, C * r * r)))


# ================================================================== backward
@functools.lru_cache(maxsize=None)
def _dyadic_d(case):
    """d [B,C,gh,gw]: multiples of 1/64 in [-4, 4] that are never 0 or +-DELTA, then a handful of exact 0 and +-DELTA entries."""
    r, C, H, W, gh, gw, B = case
    g = torch.Generator().manual_seed(H * 31 + gh * 7 + gw + r)
    n = B * C * gh * gw
    k = torch.randint(1, 257, (n,), generator=g)                     # 1 .. 256
    k = torch.where(k == int(DELTA * 64), k + 1, k)                  # never DELTA itself
    sgn = torch.randint(0, 2, (n,), generator=g) * 2 - 1
    d = (k * sgn).to(torch.float32) / 64.0
    assert float(d.abs().min()) >= 1.0 / 64 and float((d.abs() - DELTA).abs().min()) >= 1.0 / 64
    special = torch.tensor([0.0, DELTA, -DELTA, -0.0, DELTA, -DELTA])
    pos = torch.randperm(n, generator=g)[:min(n, 6)]
    d[pos] = special[:pos.numel()]
    return d.reshape(B, C, gh, gw)


@pytest.mark.parametrize("kind,param", KINDS)
@pytest.mark.parametrize("which", ["dpred", "gloss", "both"])
@pytest.mark.parametrize("case", CASES, ids=_name)
def test_head_loss_bwd_vs_float64(case, which, kind, param):
    dev = _gpu()
    r, C, H, W, gh, gw, B = case
    HH, WW = H * r, W * r
    resize = _is_resize(case)
    dc = _dyadic_d(case)
    assert int((dc == 0).sum()) >= 1 and int((dc.abs() == DELTA).sum()) >= 1
    torch.manual_seed(H * 7 + r + gw)
    dpredc = torch.randn(B, C, HH, WW) if which != "gloss" else None
    glossc = torch.tensor(0.37) if which != "dpred" else None
    dpred = dpredc.to(dev) if dpredc is not None else None
    gloss = glossc.to(dev) if glossc is not None else None
    dsave = pred = gt = None
    if which != "dpred":                                             # without gloss none of them is read: NULL
        if resize:
            dsave = dc.to(dev)
        else:                                                        # pred = d + gt with integer counts: pred - gt == d exactly
            gtc = torch.poisson(torch.full((B, C + 1, gh, gw), 0.7), generator=torch.Generator().manual_seed(gh + 3))
            gt = gtc.to(dev)[:, :C]                                  # batch stride larger than C*gh*gw
            predc = dc + gtc[:, :C]
            assert torch.equal(predc - gtc[:, :C], dc)
            pred = predc.to(dev)
    dlr = Guarded(B * C * HH * WW, dev)
    _bwd_call(case, dpred, dsave, pred, gt, gloss, kind, param, dlr)
    got = dlr.cpu((B, H, W, C * r * r))
    if which == "dpred":
        assert torch.equal(got, R.unshuffle_to_nhwc(dpredc, r, 1))   # a pure permutation
        return
    # ATen: fp32 autograd of the loss (and of the bicubic resize) at the same d
    zeros = torch.zeros(B, C, gh, gw)
    leaf = torch.zeros(B, C, HH, WW, requires_grad=True)
    sp = F.interpolate(leaf, size=(gh, gw), mode="bicubic", align_corners=False) if resize else leaf
    assert torch.equal((sp + dc).detach(), dc)
    (g,) = torch.autograd.grad(_aten_loss(kind, param, sp + dc, zeros), leaf, glossc)
    if dpredc is not None:
        g = dpredc + g
    ref = R.shuffle_to_hr(HL.bwd(dpredc, dc, glossc, r, HH, WW, kind, param), r)      # in the prediction's layout (a permutation)
    gotp = R.shuffle_to_hr(got, r)
    name = "head_loss_bwd %s %s %s" % (kind, _name(case), which)
    if resize:
        e = _edges(gotp.shape)
        vs_aten(name + " border", gotp, g, ref, e)
        vs_aten(name + " interior", gotp, g, ref, ~e)
    else:
        vs_aten(name, gotp, g, ref)
    if which == "gloss":                                             # the pinned entries, exactly: sign(0) = 0, +-delta at the boundary
        if not resize:
            coef = torch.tensor(0.37) / torch.tensor(float(B * C * gh * gw))
            at = lambda v: gotp[dc == v]
            assert bool((at(0.0) == 0).all())
            if kind != "charbonnier":
                hi = 1.0 if kind == "l1" else DELTA
                assert torch.equal(at(DELTA), (coef * hi).expand_as(at(DELTA)))
                assert torch.equal(at(-DELTA), (coef * -hi).expand_as(at(-DELTA)))
    dlr2 = Guarded(B * C * HH * WW, dev)                             # run-to-run identical
    _bwd_call(case, dpred, dsave, pred, gt, gloss, kind, param, dlr2)
    assert torch.equal(dlr2.cpu((B, H, W, C * r * r)), got)


def test_head_loss_refuses_on_the_device():
    dev = _gpu()
    a = torch.ones(64, device=dev)
    p = a.data_ptr()
    pred, dsave, part, loss, dlr = Guarded(64, dev), Guarded(64, dev), Guarded(2048, dev), Guarded(1, dev), Guarded(64, dev)
    HUBER = _kind_const("huber")
    ok = [p, 1, 1, 2, 2, 2, p, 4, 4, 2, 1, p, 12, 3, 4, pred.ptr(), dsave.ptr(), part.ptr(), loss.ptr(), HUBER, 1.0]
    for i, v in ((0, None), (11, None), (18, None), (13, 0), (19, 0), (19, 4), (20, 0.0), (20, float("nan")), (20, float("inf"))):
        args = list(ok)
        args[i] = v
        refused("_head_loss_fwd", "bmc_head_loss_fwd", *args)
    okb = [p, p, p, p, 12, p, 1, 1, 2, 2, 2, 3, 4, HUBER, 1.0, dlr.ptr()]
    for i, v in ((1, None), (15, None), (11, 0), (13, 9), (14, -1.0)):
        args = list(okb)
        args[i] = v
        refused("_head_loss_bwd", "bmc_head_loss_bwd", *args)
    assert all(g.untouched() for g in (pred, dsave, part, loss, dlr))


# ================================================================== the model and the steps
MODEL_KINDS = [("l1", 0.0), ("huber", 0.5), ("charbonnier", EPS)]
GT_SIZES = [(22, 35), (24, 36)]                                      # another size / the prediction's own (LR 6x9, x4)


@functools.lru_cache(maxsize=None)
def _plain(size):
    dev = _gpu()
    m, inp, gt, n_c, scale = _plain_case(dev)
    if size != tuple(gt.shape[-2:]):
        torch.manual_seed(12)
        gt = torch.poisson(torch.full(tuple(gt.shape[:3]) + size, 0.3)).to(dev)
    return m, inp, gt, n_c, scale


def _compare(tag, lf, gf, lu, gu):
    rel = abs(lf.item() - lu.item()) / abs(lu.item())
    worst = max(rel_l2(gf[k], gu[k]) for k in gu)
    print("MODEL %s fused %.8f unfused %.8f rel %.2e  grads %d worst rel-L2 %.3e" % (tag, lf.item(), lu.item(), rel, len(gu), worst))
    assert rel <= 1e-5, (tag, lf.item(), lu.item())
    assert len(gf) == len(gu) > 0
    for k in gu:
        d = rel_l2(gf[k], gu[k])
        assert d <= 1e-4, (tag, k, d)


@pytest.mark.parametrize("kind,param", MODEL_KINDS)
@pytest.mark.parametrize("size", GT_SIZES, ids=lambda s: "gt%dx%d" % s)
def test_plain_model_fused_equals_unfused_and_recompute_is_bit_identical(size, kind, param, monkeypatch):
    from bmc_hip import lib, ops
    m, inp, gt, n_c, scale = _plain(size)
    L = _loss_obj(kind, param)
    lu, _, gu = _step(m, inp, gt, n_c, scale, loss_fn=lambda a, b: L(a, b))          # the unfused chain, the same loss object
    monkeypatch.setattr(lib, "_bicubic_fwd", _raise("bmc_bicubic_resize_fwd"))       # ... whose entry points now raise
    monkeypatch.setattr(ops, "head", _raise("ops.head"))
    monkeypatch.setattr(ops, "head_mse", _raise("ops.head_mse"))
    monkeypatch.setattr(ops, "head_resize_mse", _raise("ops.head_resize_mse"))
    lf, mf, gf = _step(m, inp, gt, n_c, scale, loss_fn=L)
    _compare("plain %s gt%dx%d" % (kind, *size), lf, gf, lu, gu)
    l1, m1, g1 = _step(m, inp, gt, n_c, scale, loss_fn=L, recompute=True)
    assert torch.equal(lf, l1) and torch.equal(mf, m1)
    for k in gf:
        assert torch.equal(gf[k], g1[k]), k


@pytest.mark.parametrize("size", GT_SIZES, ids=lambda s: "gt%dx%d" % s)
def test_valid_step_with_a_loss_object_is_forward_only(size, monkeypatch):
    from bmc_hip import lib, loss_lib, ops
    from train_step import valid_step
    m, inp, gt, n_c, scale = _plain(size)
    L = _loss_obj("charbonnier", EPS)
    want, _ = valid_step(m, inp, gt, n_c, scale, plain=True, loss=lambda a, b: L(a, b))      # the unfused chain
    saves = []
    real = loss_lib._head_loss_fwd

    def spy(*args):
        saves.append(args[16])
        return real(*args)

    monkeypatch.setattr(loss_lib, "_head_loss_fwd", spy)
    monkeypatch.setattr(lib, "_bicubic_fwd", _raise("bmc_bicubic_resize_fwd"))
    monkeypatch.setattr(ops, "head", _raise("ops.head"))
    for mode in (True, False):
        m.train(mode)
        loss, last = valid_step(m, inp, gt, n_c, scale, plain=True, loss=L)
        assert m.training is mode and not loss.requires_grad and not last.requires_grad
        assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())
    assert all(p.grad is None for p in m.parameters())
    assert len(saves) == 6 and all(s is None for s in saves)         # 2 x 3 windows: nothing of the ground truth's size is stored


def test_bmcnet_golden_resize_branch_with_huber(monkeypatch):
    """One BMCNet step on the golden bmcnet_resize.npz operands (28x56 prediction, 28x54 ground truth) with Huber: the fused
    head against the unfused chain with the same loss object, at the plain model's bars."""
    dev = _gpu()
    from bmc_hip import lib, ops
    from train_step import bptt_step
    L = _loss_obj("huber", 1.0)
    out = {}
    for path in ("unfused", "fused"):
        m, z, frames, gts, n_c, scale = _golden_model(dev)
        opt = torch.optim.SGD(m.parameters(), lr=0.0)
        if path == "fused":
            monkeypatch.setattr(lib, "_bicubic_fwd", _raise("bmc_bicubic_resize_fwd"))
            monkeypatch.setattr(ops, "head", _raise("ops.head"))
            monkeypatch.setattr(ops, "head_resize_mse", _raise("ops.head_resize_mse"))
        loss, _ = bptt_step(m, opt, frames, gts, n_c, scale, loss_fn=L if path == "fused" else (lambda a, b: L(a, b)))
        out[path] = (loss, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    assert len(out["fused"][1]) >= 40
    _compare("BMCNet huber golden", *out["fused"], *out["unfused"])
