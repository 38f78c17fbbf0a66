"""bmc_ssim_loss_fwd / _bwd (include/bmc_hip_ssim.h, csrc/ssim_loss.hip: 1 - mean SSIM over the 7x7 windows inside the image, float64
on the float32 inputs, and its gradient) alone against their float64 restatement (tests/ssim_loss_ref.py), ops.ssim_loss, and the
training / validation step that takes them when loss_fn is a bmc_hip.losses.SSIM or Mix object.

Kernel tests go through ctypes into guarded buffers.  The bars are not constants: for every input the loss and the gradient are
evaluated twice in float64 -- the restatement in the kernels' summation order, and the conv2d formulation with autograd -- and
their distance (d for the loss, d_g elementwise for the gradient) is float64's own sensitivity to summation order on that input:
    |L_hip - L_64| <= 2^-23 |L_64| + 8 d          (d = 1e-15 where the two agree bit for bit)
    |g_hip - g_64| <= 2^-23 |g_64| + 8 d_g        elementwise
with L_64, g_64 the restatement's.  torch.autograd.gradcheck is not used: the inputs are float32; the comparison above replaces it.

Shapes (TH x TW the forward tile in window positions, PH x PW the backward tile in pixels, read from the binding): 7x7 one
position; 7x8, 8x7 one ragged row / column; 13x9 every pixel's window set clipped at a border; (TH + 7) x (2 TW + 9) ragged forward
tiles in both directions; (2 PH + 1) x (PW + 5) the backward's apron crossing tile edges and clipped by the image.  B x C from
{1x2, 3x2, 2x1}; the ground truth contiguous and as a slice gt_cnt[:, i] with a batch stride; data ranges 1, 8, 255.  Inputs are
count-like (ssim_loss_ref.make_pair)."""
import functools
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity_bars as PB
import quality_ref as Q
import ssim_loss_ref as SR
from bmc_hip import ssim_lib
from bmc_hip.losses import L1, SSIM, Mix
from test_gpu_head_loss import _plain
from test_gpu_head_resize import _raise, _step
from test_gpu_r2 import _gpu, _restore_math_mode, rel_l2  # noqa: F401
from test_gpu_streaming_kernels import GUARD, SENT, Guarded

pytestmark = pytest.mark.gpu

TH, TW, PH, PW = ssim_lib.TILE_H, ssim_lib.TILE_W, ssim_lib.BWD_TILE_H, ssim_lib.BWD_TILE_W
SHAPES = SR.shapes(TH, TW, PH, PW)
BATCHES = [(1, 2), (3, 2), (2, 1)]
RANGES = [1.0, 8.0, 255.0]
LAYOUTS = ["contiguous", "sliced"]
GLOSS = float(np.float32(-0.3))                              # the non-trivial upstream gradient (a float32 value)
U32 = 2.0 ** -23


def _bc(shape, R):
    """The B x C of a case: every shape meets all three, one per data range."""
    return BATCHES[(SHAPES.index(shape) + RANGES.index(R)) % 3]


@functools.lru_cache(maxsize=None)
def _ref(shape, R):
    """One input per (shape, data range) and everything float64 says about it; computed once, shared, never written to."""
    B, C = _bc(shape, R)
    x, y = SR.make_pair(B, C, *shape, seed=1000 * shape[0] + 10 * shape[1] + int(R))
    L, (Lc, gc) = SR.loss(x, y, R, TH, TW), SR.conv2d_loss_and_grad(x, y, R)
    out = dict(B=B, C=C, x=x, y=y, L=L, d=abs(L - Lc) or 1e-15)
    for tag, gl in (("g1", 1.0), ("gs", GLOSS)):
        g = SR.grad(x, y, R, gl)
        out[tag], out["d_" + tag] = g, float(np.abs(g - gc * gl).max())
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _device_pair(ref, layout, dev):
    """-> x, y on the device; 'sliced': y = gt_cnt[:, 1] of a [B, 3, C, h, w] tensor (a batch stride of 3 C h w), its neighbours
    filled with a value that would show in any result."""
    x, y = torch.tensor(ref["x"]).to(dev), torch.tensor(ref["y"]).to(dev)
    if layout == "sliced":
        seq = torch.full((y.shape[0], 3) + tuple(y.shape[1:]), 1e6, device=dev)
        seq[:, 1] = y
        y = seq[:, 1]
        assert not y.is_contiguous() or y.shape[0] == 1
    return x, y


class Guarded64:
    """Guarded for float64 scratch."""

    def __init__(self, n, dev):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float64, device=dev)

    def ptr(self):
        return self.buf[GUARD:].data_ptr()

    def guards_intact(self):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        return bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + self.n:] == SENT).all())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENT).all())


def _call(fn, what, *args):
    from bmc_hip import lib, ops
    lib.call(fn, what, *args, ops._stream())


def _fwd(x, y, R, tiles, loss):
    B, C, h, w = x.shape
    _call(ssim_lib._ssim_loss_fwd, "bmc_ssim_loss_fwd", x.data_ptr(), y.data_ptr(), y.stride(0), B, C, h, w, R, tiles.ptr(), loss.ptr())


def _bwd(x, y, R, gloss, dx):
    B, C, h, w = x.shape
    _call(ssim_lib._ssim_loss_bwd, "bmc_ssim_loss_bwd", x.data_ptr(), y.data_ptr(), y.stride(0), gloss.data_ptr(), B, C, h, w, R, dx.ptr())


# ================================================================== the kernels alone
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("R", RANGES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_ssim_loss_fwd_vs_float64(shape, R, layout):
    dev = _gpu()
    ref = _ref(shape, R)
    x, y = _device_pair(ref, layout, dev)
    ntiles = ref["B"] * ref["C"] * ssim_lib.fwd_tiles(*shape)
    tiles, loss, loss2 = Guarded64(ntiles, dev), Guarded(1, dev), Guarded(1, dev)
    _fwd(x, y, R, tiles, loss)
    got = loss.cpu()
    L, d = ref["L"], ref["d"]
    err, bar = abs(float(got[0]) - L), U32 * abs(L) + 8 * d
    print("FWD %dx%d B%dC%d R=%g %s: L_64 %.17g  hip %.9g  |diff| %.3e  d %.3e  bar %.3e  (float32(L_64) %s)" % (
        *shape, ref["B"], ref["C"], R, layout, L, float(got[0]), err, d, bar, "==" if np.float32(L) == got.numpy()[0] else "!="))
    assert err <= bar
    assert tiles.guards_intact()
    _fwd(x, y, R, tiles, loss2)                                # run to run: the same bits
    assert torch.equal(loss2.cpu().view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("R", RANGES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_ssim_loss_bwd_vs_float64(shape, R, layout):
    dev = _gpu()
    ref = _ref(shape, R)
    x, y = _device_pair(ref, layout, dev)
    for tag, gl in (("g1", 1.0), ("gs", GLOSS)):
        gloss = torch.tensor(gl, dtype=torch.float32, device=dev)
        dx = Guarded(x.numel(), dev, init=torch.full((x.numel(),), float("nan")))
        _bwd(x, y, R, gloss, dx)
        got = dx.cpu(x.shape).double().numpy()                # (asserts the guards)
        assert np.isfinite(got).all(), "an element of dx was not written"
        g, d_g = ref[tag], ref["d_" + tag]
        excess = np.abs(got - g) - (U32 * np.abs(g) + 8 * d_g)
        print("BWD %dx%d B%dC%d R=%g %s gloss=%g: max|g_64| %.3e  max|diff| %.3e  d_g %.3e  worst excess over the bar %.3e  "
              "(%d of %d elements are float32(g_64))" % (*shape, ref["B"], ref["C"], R, layout, gl, np.abs(g).max(), np.abs(got - g).max(),
                                                       d_g, excess.max(), int((got == g.astype(np.float32)).sum()), g.size))
        assert (excess <= 0).all()
        dx2 = Guarded(x.numel(), dev, init=torch.full((x.numel(),), float("nan")))
        _bwd(x, y, R, gloss, dx2)
        assert torch.equal(dx2.cpu().view(torch.int32), dx.cpu().view(torch.int32))


@pytest.mark.parametrize("case", ["same", "zeros"])
def test_exact_cases(case):
    """x == y bit for bit: S = 1 at every position, loss 0 and a gradient of exact zeros; so for a pair of empty images."""
    dev = _gpu()
    from bmc_hip import ops
    for shape in ((9, 13), (2 * PH + 1, PW + 5)):
        y = torch.tensor(SR.make_pair(2, 2, *shape, seed=5)[1]).to(dev) if case == "same" else torch.zeros(2, 2, *shape, device=dev)
        for R in RANGES:
            x = y.clone().requires_grad_()
            loss = ops.ssim_loss(x, y, R)
            (g,) = torch.autograd.grad(loss, x, torch.tensor(GLOSS, device=dev))
            assert float(loss.detach()) == 0.0 and not bool(g.any()), (shape, R, float(loss.detach()), float(g.abs().max()))


def test_refusals_through_the_c_abi_write_nothing():
    dev = _gpu()
    from bmc_hip import lib
    B, C, h, w = 2, 2, 9, 12
    a = torch.ones(B, C, h, w, device=dev)
    one = torch.ones((), device=dev)
    tiles, loss, dx = Guarded64(B * C, dev), Guarded(1, dev), Guarded(a.numel(), dev)
    p = a.data_ptr()
    fwd = dict(x=p, y=p, ybs=C * h * w, B=B, C=C, h=h, w=w, R=1.0, tiles=tiles.ptr(), loss=loss.ptr())
    bwd = dict(x=p, y=p, ybs=C * h * w, gloss=one.data_ptr(), B=B, C=C, h=h, w=w, R=1.0, dx=dx.ptr())
    common = (dict(x=None), dict(y=None), dict(h=6), dict(w=6), dict(B=1 << 12, C=1 << 12, h=8, w=8, ybs=1 << 18), dict(R=0.0),
              dict(R=-8.0), dict(R=float("inf")), dict(R=float("nan")), dict(ybs=C * h * w - 1))
    for fn, what, ok, more in ((ssim_lib._ssim_loss_fwd, "bmc_ssim_loss_fwd", fwd, (dict(tiles=None), dict(loss=None), dict(tiles=tiles.ptr() + 4))),
                               (ssim_lib._ssim_loss_bwd, "bmc_ssim_loss_bwd", bwd, (dict(gloss=None), dict(dx=None)))):
        for kw in common + more:
            with pytest.raises(RuntimeError, match=what):
                _call(fn, what, *{**ok, **kw}.values())
            assert fn(*{**ok, **kw}.values(), None) == -1 and what.encode() in lib.bmc_last_error()      # the usual error code
    assert tiles.untouched() and loss.untouched() and dx.untouched()


# ================================================================== ops.ssim_loss
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ops_ssim_loss_is_the_two_entry_points(layout, monkeypatch):
    """The autograd Function gives the bits of the direct calls, hands a sliced ground truth over with its batch stride (no copy),
    saves pred and gt only, and under no_grad allocates the scalar alone once the tile scratch of the shape is cached."""
    dev = _gpu()
    from bmc_hip import ops
    shape, R = SHAPES[4], 8.0
    ref = _ref(shape, R)
    x, y = _device_pair(ref, layout, dev)
    tiles, loss, dx = Guarded64(x.shape[0] * x.shape[1] * ssim_lib.fwd_tiles(*shape), dev), Guarded(1, dev), Guarded(x.numel(), dev)
    gloss = torch.tensor(GLOSS, device=dev)
    _fwd(x, y, R, tiles, loss)
    _bwd(x, y, R, gloss, dx)
    seen = []
    real = ssim_lib._ssim_loss_fwd
    monkeypatch.setattr(ssim_lib, "_ssim_loss_fwd", lambda *a: (seen.append(a[1:3]), real(*a))[1])
    xg = x.clone().requires_grad_()
    got = ops.ssim_loss(xg, y, R)
    assert got.dtype == torch.float32 and got.dim() == 0 and got.requires_grad
    assert seen == [(y.data_ptr(), y.stride(0))]
    assert torch.equal(got.detach().cpu().reshape(1), loss.cpu())
    saved = got.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == xg.data_ptr() and saved[1].data_ptr() == y.data_ptr()
    (g,) = torch.autograd.grad(got, xg, gloss)
    assert torch.equal(g.cpu().reshape(-1), dx.cpu())
    with torch.no_grad():
        ops.ssim_loss(x, y, R)                                   # (the scratch of this shape and stream is cached by now)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        again = ops.ssim_loss(x, y, R)
        assert torch.cuda.max_memory_allocated(dev) - before <= 512 and not again.requires_grad
    assert torch.equal(again.cpu().reshape(1), loss.cpu())
    with pytest.raises(RuntimeError, match="one shape"):
        ops.ssim_loss(x, y[:, :, :-1], R)
    with pytest.raises(ValueError, match="at least 7 x 7"):
        ops.ssim_loss(x[:, :, :6], y[:, :, :6], R)


@pytest.mark.parametrize("R", RANGES)
def test_one_minus_loss_is_image_quality_ssim(R):
    """B = 1: the loss is one minus what MultiStreamSR(quality=...) reports for the image (bmc_slot_quality with a constant range),
    within the float32 rounding of the loss (half an ulp) and the bar tests/quality_ref.py sets between two float64 orders."""
    dev = _gpu()
    from bmc_hip import encodings, ops
    for shape in (SHAPES[3], SHAPES[4]):
        x, y = (torch.tensor(t).to(dev) for t in SR.make_pair(1, 2, *shape, seed=shape[0]))
        L = float(ops.ssim_loss(x, y, R))
        ssim = encodings.image_quality(x, y, data_range=R)["ssim"][0]
        assert abs((1.0 - L) - ssim) <= 0.5 * float(np.spacing(np.float32(L))) + Q.SSIM_BAR, (shape, R, L, ssim)


def test_captured_graph_replay_gives_the_eager_bits():
    dev = _gpu()
    from bmc_hip import ops
    ref = _ref(SHAPES[5], 8.0)
    x, y = _device_pair(ref, "sliced", dev)
    x.requires_grad_()
    gloss = torch.tensor(GLOSS, device=dev)
    loss = ops.ssim_loss(x, y, 8.0)
    (g,) = torch.autograd.grad(loss, x, gloss)
    # torch's capture protocol: no autograd graph made outside the capture may reach into it.  x's gradient accumulator carries
    # the stream it was made on and lives as long as a graph that uses x; kept alive from the eager call above it would make the
    # engine hand the captured gradient over to the default stream, which cannot take part in a capture.
    loss = loss.detach()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm on a side stream, as torch asks before a capture
        for _ in range(2):
            torch.autograd.grad(ops.ssim_loss(x, y, 8.0), x, gloss)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gl = ops.ssim_loss(x, y, 8.0)
        (gg,) = torch.autograd.grad(gl, x, gloss)
    for _ in range(2):
        gl.fill_(float("nan"))
        gg.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gl.view(torch.int32), loss.detach().view(torch.int32)) and torch.equal(gg.view(torch.int32), g.view(torch.int32))


# ================================================================== the model and the steps
GT_SIZES = [(22, 35), (24, 36)]                                      # another size (the resize branch) / the prediction's own
OBJECTS = {"ssim": lambda: SSIM(8.0), "l1+ssim": lambda: Mix(L1(), SSIM(8.0))}


def _compare(tag, lf, gf, lu, gu):
    """The bars of the fused-against-unfused model tests (tests/test_gpu_head_loss.py: 1e-5 on the loss, relative, 1e-4 rel-L2 on
    every gradient), inside tests/parity_bars.py's contract."""
    PB.within(abs(lf.item() - lu.item()) / abs(lu.item()), 1e-5, PB.CONTRACT_SR, "%s loss %.8f / %.8f" % (tag, lf.item(), lu.item()))
    assert len(gf) == len(gu) > 0
    worst = max(gu, key=lambda k: rel_l2(gf[k], gu[k]))
    for k in gu:
        assert rel_l2(gf[k], gu[k]) <= 1e-4, (tag, k)
    PB.within(rel_l2(gf[worst], gu[worst]), 1e-4, PB.CONTRACT_GRAD, "%s worst of %d gradients (%s)" % (tag, len(gu), worst))


@pytest.mark.parametrize("name", sorted(OBJECTS))
@pytest.mark.parametrize("size", GT_SIZES, ids=lambda s: "gt%dx%d" % s)
def test_plain_model_device_path_equals_unfused_and_recompute_is_bit_identical(size, name, monkeypatch):
    from bmc_hip import ops
    m, inp, gt, n_c, scale = _plain(size)
    L = OBJECTS[name]()
    lu, _, gu = _step(m, inp, gt, n_c, scale, loss_fn=lambda a, b: L(a, b))          # the unfused chain, the same loss object
    # the prediction, two windows with the state carried: bit for bit the unfused model's
    B, _, _, H, W = inp.shape
    z = lambda c: torch.zeros(B, c, H, W, device=inp.device)
    su = sf = (z(n_c), z(2 * scale * scale))
    with torch.no_grad():
        for i in range(2):
            x = inp[:, i:i + 2].transpose(1, 2)
            su = tuple(m(x, *su, i == 0))
            *sf, value = m.forward_loss(x, *sf, i == 0, gt[:, i + 1], loss=L)
            assert torch.equal(sf[-1], su[-1]) and torch.equal(sf[0], su[0])
            want = L(ops.bicubic_resize(su[-1], size), gt[:, i + 1])
            assert abs(float(value) - float(want)) <= 1e-5 * abs(float(want))
    calls = []
    real = ssim_lib._ssim_loss_bwd
    monkeypatch.setattr(ssim_lib, "_ssim_loss_bwd", lambda *a: (calls.append(1), real(*a))[1])
    lf, mf, gf = _step(m, inp, gt, n_c, scale, loss_fn=L)
    assert len(calls) == 3                                           # one backward launch per window
    _compare("plain %s gt%dx%d" % (name, *size), lf, gf, lu, gu)
    l1, m1, g1 = _step(m, inp, gt, n_c, scale, loss_fn=L, recompute=True)
    assert torch.equal(lf, l1) and torch.equal(mf, m1)
    for k in gf:
        assert torch.equal(gf[k], g1[k]), k


@pytest.mark.parametrize("size", GT_SIZES, ids=lambda s: "gt%dx%d" % s)
def test_valid_step_with_ssim_is_forward_only(size, monkeypatch):
    from train_step import valid_step
    m, inp, gt, n_c, scale = _plain(size)
    L = SSIM()
    want, _ = valid_step(m, inp, gt, n_c, scale, plain=True, loss=lambda a, b: L(a, b))      # the unfused chain
    monkeypatch.setattr(ssim_lib, "_ssim_loss_bwd", _raise("bmc_ssim_loss_bwd"))
    calls = []
    real = ssim_lib._ssim_loss_fwd
    monkeypatch.setattr(ssim_lib, "_ssim_loss_fwd", lambda *a: (calls.append(1), real(*a))[1])
    for mode in (True, False):
        m.train(mode)
        loss, last = valid_step(m, inp, gt, n_c, scale, plain=True, loss=L)
        assert m.training is mode and not loss.requires_grad and not last.requires_grad
        assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())
    assert all(p.grad is None for p in m.parameters()) and len(calls) == 6          # 2 x 3 windows


def test_mse_and_l1_steps_never_touch_the_new_module(monkeypatch):
    """F.mse_loss and L1() take the code path they took before: with bmc_hip.ssim_lib unimportable and every new function of ops
    raising, their steps run and give the bits they give otherwise."""
    from bmc_hip import ops
    m, inp, gt, n_c, scale = _plain(GT_SIZES[0])
    before = [_step(m, inp, gt, n_c, scale), _step(m, inp, gt, n_c, scale, loss_fn=L1())]
    import bmc_hip
    monkeypatch.setitem(sys.modules, "bmc_hip.ssim_lib", None)        # with the package's attribute gone too,
    monkeypatch.delattr(bmc_hip, "ssim_lib")                          # `from . import ssim_lib` now raises ImportError
    monkeypatch.setattr(ops, "_ssim_lib", None)
    for name in ("ssim_loss", "head_structural_loss"):
        monkeypatch.setattr(ops, name, _raise("ops." + name))
    with pytest.raises(ImportError):
        ops._ssim()
    after = [_step(m, inp, gt, n_c, scale), _step(m, inp, gt, n_c, scale, loss_fn=L1())]
    for (l0, m0, g0), (l1, m1, g1) in zip(before, after):
        assert torch.equal(l0, l1) and torch.equal(m0, m1) and all(torch.equal(g0[k], g1[k]) for k in g0)


def test_a_lambda_around_the_object_selects_the_unfused_chain(monkeypatch):
    from bmc_hip import ops
    m, inp, gt, n_c, scale = _plain(GT_SIZES[0])
    L = SSIM(8.0)
    monkeypatch.setattr(ops, "ssim_loss", _raise("ops.ssim_loss"))
    loss, _, grads = _step(m, inp, gt, n_c, scale, loss_fn=lambda a, b: L(a, b))
    assert bool(torch.isfinite(loss)) and len(grads) > 0
    with pytest.raises(AssertionError, match="ops.ssim_loss was called"):
        _step(m, inp, gt, n_c, scale, loss_fn=L)
