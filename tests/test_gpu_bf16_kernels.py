"""GPU tests of the bf16 arithmetic mode (ops.set_math("bf16"), BMC_MATH_BF16) layer by layer (-m gpu): every kernel that runs
in this mode -- `conv_bf_kernel<TAPS, BN, TH, 1>` (all 8 tile instantiations), `pgemm_bf_kernel<9|1, 1, TAB>` (both sides of the
tap-row rule, the pointer-table kernels of merged weight gradients), the one-plane weight split -- against the float64 oracle
of the mode's contract, `oracle.bmc_oracle.conv2d` under `operand_rounding("bf16")`: every contraction (forward, data
gradient, weight gradient) rounds BOTH operands to bf16 (RNE of the float32 value) and accumulates exactly; bias, residual,
ReLU, mask, accumulate and the bias gradient stay unrounded.

A single layer whose inputs are float32 tensors rounds exactly as that reference does, so each comparison checks two things:
  * bar: rel-L2 to the ROUNDED float64 reference below BAR (the bar of test_gpu_parity.py::test_math_modes_vs_float64): what
    is left is fp32 accumulation;
  * resolution: the distance to the UNROUNDED float64 reference is at least RESOLUTION x that error -- the kernel really
    rounds both operands, and the test can tell (a kernel that ran fp32 or bf16x6 would pass the bar and fail here).
The model-level bf16 tests resolve ~1e-4 at best; these hold the kernels ~1000x tighter."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import bmc_oracle as O  # noqa: E402
from test_gpu_parity import _gpu, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

# MI355X, measured: 1.4e-8 .. 2.4e-7 over every bf16 comparison of parts 1-5, 1.0e-7 .. 4.0e-7 for bf16x6 against the
# unrounded reference, 1.2e-7 .. 3.0e-7 merged vs unmerged; the unrounded reference sits 1.5e-3 .. 2.4e-3 away (x1e4 .. x1.6e5)
BAR = 3e-6            # rel-L2 to the rounded reference (test_math_modes_vs_float64)
BAR_X6 = 3e-6         # bf16x6 against the unrounded reference (fp32-class: test_math_modes_vs_float64's bar for that mode)
RESOLUTION = 30.0     # error vs the unrounded reference >= RESOLUTION x error vs the rounded one
BAR_MERGE = 2e-6      # merged vs unmerged weight gradients (test_merged_weight_gradients_past_one_pointer_table has 2e-5)
BAR_WIDE = 8e-6       # max |err| / sum |r(x)| |r(w)| on operands over 2^-40 .. 2^40 (measured 7.6e-7 3x3, 3.5e-7 1x1)


@pytest.fixture(autouse=True)
def _restore_modes():
    yield
    from bmc_hip import ops
    ops.set_math(os.environ.get("BMC_MATH", "fp32"))


@pytest.fixture
def pgemm_log(monkeypatch):
    """Every bmc_pgemm launch of the test: (math, tap_groups, nsplit, taps, table operands, B) read off its argument block."""
    from bmc_hip import lib
    log, real = [], lib.call

    def call(fn, what, *args):
        if what == "bmc_pgemm":
            p = args[0]._obj
            log.append(dict(math=p.math, tap_groups=p.tap_groups, nsplit=p.nsplit, taps=p.taps, table=p.a.batch_mod == -1, B=p.B))
        return real(fn, what, *args)

    monkeypatch.setattr(lib, "call", call)
    return log


# ------------------------------------------------------------------ the tile rule of bmc_conv (csrc/conv.hip, bmc_conv)
def conv_tile(B, H, W, Cout, cus):
    """(BN, TH) that bmc_conv gives a launch of the direct / bf16-plane kernels: 8 x 16-pixel x 128-channel tiles when there
    are at least 2 per CU, else 4-row tiles, else 4-row x 64-channel tiles; Coutpad 32 takes 32-channel tiles."""
    cp = 32 if Cout <= 32 else (Cout + 127) // 128 * 128
    count = lambda th, bn: B * ((W + 15) // 16) * ((H + th - 1) // th) * (cp // bn)
    bn, th = (32, 8) if cp == 32 else (128, 8)
    if bn == 128 and count(8, 128) < 2 * cus:
        th = 4
        if count(4, 128) < 2 * cus:
            bn = 64
    return bn, th


ALL_BF_TILES = {(t, bn, th) for t in (9, 1) for bn, th in ((32, 8), (64, 4), (128, 4), (128, 8))}

# part 1: (taps, BN, TH) the forward launch must take, sources, Cout, image (H, W), bias, relu, residual.  The batch comes
# from the device's CU count (conv_batch): the smallest one whose forward launch takes that tile.
CONV_CASES = [
    (9, 32, 8, [16, 32], 16, (13, 21), False, True, False),             # simple epilogue (no bias, ReLU only)
    (1, 32, 8, [48, 16, 16], 16, (19, 37), True, False, True),          # general epilogue: residual
    (9, 64, 4, [128], 80, (19, 37), True, True, False),                 # bias on two column tiles: general epilogue
    (1, 64, 4, [16, 32, 48, 16, 16], 48, (11, 29), False, True, False),  # five sources, simple epilogue
    (9, 128, 4, [32, 16], 160, (29, 61), True, False, True),
    (1, 128, 4, [128, 128], 48, (23, 45), True, True, False),           # bias in the accumulators: simple epilogue with bias
    (9, 128, 8, [48], 160, (35, 61), False, True, False),
    (1, 128, 8, [16, 48, 32], 80, (37, 75), True, True, True),          # residual + ReLU: general epilogue
]


def conv_batch(case, cus):
    taps, bn, th, cins, cout, (H, W) = case[:6]
    for B in range(1, 65):
        if conv_tile(B, H, W, cout, cus) == (bn, th):
            return B
    raise AssertionError("no batch gives tile %s for %s at %d CUs" % ((bn, th), case, cus))


def conv_cases_tiles(cus):
    return {(c[0],) + conv_tile(conv_batch(c, cus), c[5][0], c[5][1], c[4], cus) for c in CONV_CASES}


# part 4: weight-gradient launches on both sides of ops.pgemm_raw's tap-row rule (one tap row per workgroup, tap_groups = 3,
# where a workgroup would get fewer than TAP_SPLIT_TILES pixel tiles): (B, H, W, sources, Cout, G, tap_groups expected)
WGRAD_CASES = [
    (1, 13, 21, [16, 32], 16, 1, 3),
    (2, 9, 35, [48], 48, 2, 3),
    (2, 11, 27, [32, 16, 16], 160, 1, 3),
    (4, 61, 93, [128, 32, 16], 160, 1, 1),
    (5, 61, 93, [128, 128, 32, 16], 48, 1, 1),
    (4, 61, 93, [128, 32, 16], 160, 2, 1),
]


# ------------------------------------------------------------------ reference
def _f64(t):
    return t.detach().cpu().double()


def conv_reference(srcs, w, b, res, go, mask, G, B, rounded):
    """float64 CPU reference of one ops.conv launch: srcs = [(tensor NCHW, shift, mod)] read as launch batch i -> image
    (i + shift) % mod, res the same (or None), per-group weights w [G, Cout, Cin, k, k] (G = 1: [Cout, Cin, k, k]), bias [G, Cout] /
    [Cout].  mask: the ReLU gate the kernel applied (bool NCHW) or None.  -> (y, [dx], dw, db, dres)."""
    xs = [_f64(t).requires_grad_() for t, _, _ in srcs]
    wd = _f64(w).requires_grad_()
    bd = _f64(b).requires_grad_() if b is not None else None
    rd = _f64(res[0]).requires_grad_() if res is not None else None
    gather = lambda t, shift, mod: t[[(i + shift) % (mod if mod is not None else B) for i in range(B)]]
    inp = torch.cat([gather(t, s, m) for t, (_, s, m) in zip(xs, srcs)], 1)
    bpg = B // G
    w5 = wd.reshape(G, wd.shape[-4] if wd.dim() >= 4 else wd.shape[-2], inp.shape[1], *(wd.shape[-2:] if wd.dim() >= 4 else (1, 1)))
    b2 = bd.reshape(G, -1) if bd is not None else None
    with O.operand_rounding("bf16" if rounded else None):
        z = torch.cat([O.conv2d(inp[gi * bpg:(gi + 1) * bpg], w5[gi], b2[gi] if bd is not None else None) for gi in range(G)], 0)
    if rd is not None:
        z = z + gather(rd, res[1], res[2])
    y = torch.relu(z) if mask is not None else z
    (z * mask if mask is not None else z).backward(_f64(go))
    return (y.detach(), [x.grad for x in xs], wd.grad, bd.grad if bd is not None else None, rd.grad if rd is not None else None)


def _nchw(t):
    return t.detach().permute(0, 3, 1, 2)


def check(what, got, rounded, exact=None, bar=BAR):
    """rel-L2 of `got` to the rounded reference under `bar`; with `exact`, the resolution check against the unrounded one."""
    e = rel_l2(got, rounded)
    if exact is None:
        print("    %-28s %.2e (bar %.0e)" % (what, e, bar))
    else:
        eu = rel_l2(got, exact)
        print("    %-28s %.2e (bar %.0e)   vs unrounded %.2e (x%.0f)" % (what, e, bar, eu, eu / max(e, 1e-30)))
        assert eu >= RESOLUTION * e, (what, e, eu)
    assert e < bar, (what, e, bar)
    return e


def run_conv_case(dev, cins, cout, k, B, H, W, bias, relu, res, G=1, views=None, res_view=None, wgrad=True, seed=0):
    """One ops.conv launch in bf16 with autograd (forward, dx per source, dW, db, residual gradient) against the rounded and
    unrounded float64 references.  views: per source (images, shift, mod) of its tensor, default (B, 0, None)."""
    from bmc_hip import ops
    from bmc_hip.ops import ConvSpec, View
    ops.set_math("bf16")
    g = torch.Generator().manual_seed(seed)
    views = views or [(B, 0, None)] * len(cins)
    cin = sum(cins)
    xs = [torch.randn(nb, H, W, c, generator=g) for c, (nb, _, _) in zip(cins, views)]
    wshape = (cout, cin, k, k) if G == 1 else (G, cout, cin, k, k)
    w = torch.randn(*wshape, generator=g) / (cin * k * k) ** 0.5
    b = (torch.randn(*((cout,) if G == 1 else (G, cout)), generator=g) * 0.5) if bias else None
    rv = res_view or (B, 0, None)
    r = torch.randn(rv[0], H, W, cout, generator=g) if res else None
    go = torch.randn(B, H, W, cout, generator=g)
    xs_g = [x.to(dev).requires_grad_() for x in xs]
    w_g = w.to(dev).requires_grad_(wgrad)
    b_g = b.to(dev).requires_grad_() if bias else None
    r_g = r.to(dev).requires_grad_() if res else None
    y = ops.conv([View(x, shift=s, mod=m) for x, (_, s, m) in zip(xs_g, views)], w_g, b_g, ConvSpec.dense(*cins), B=B, relu=relu,
                 residual=View(r_g, shift=rv[1], mod=rv[2]) if res else None, G=G, cache=False)
    y.backward(go.to(dev))
    torch.cuda.synchronize()
    mask = _nchw(y).cpu() > 0 if relu else None
    srcs = [(_nchw(x), s, m) for x, (_, s, m) in zip(xs, views)]
    resv = (_nchw(r), rv[1], rv[2]) if res else None
    refs = [conv_reference(srcs, w, b, resv, _nchw(go), mask, G, B, rounded) for rounded in (True, False)]
    (yr, dxr, dwr, dbr, drr), (yu, dxu, dwu, _, _) = refs
    errs = {"fwd": check("forward", _nchw(y), yr, yu)}
    for i, (xg, a, u) in enumerate(zip(xs_g, dxr, dxu)):
        errs["dx%d" % i] = check("dx of source %d (%d ch)" % (i, cins[i]), _nchw(xg.grad), a, u)
    if wgrad:
        errs["dw"] = check("dW", w_g.grad, dwr, dwu)
    if bias:
        errs["db"] = check("db", b_g.grad, dbr)
    if res:
        check("residual gradient", _nchw(r_g.grad), drr, bar=1e-12)
    return errs


# ------------------------------------------------------------------ 1. forward + data gradient, all 8 bf16 tile instantiations
def test_conv_cases_cover_every_bf16_tile():
    """The part-1 parametrization reaches all 8 (taps, BN, TH) of bmc_conv_bf_launch with a FORWARD launch on this device."""
    _gpu()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert conv_cases_tiles(cus) == ALL_BF_TILES, (cus, conv_cases_tiles(cus))


@pytest.mark.parametrize("case", CONV_CASES, ids=["t%d_bn%d_th%d" % c[:3] for c in CONV_CASES])
def test_bf16_conv_every_tile_vs_rounded_float64(case):
    """ops.conv in bf16 with autograd at ragged sizes, Cout not a multiple of the tile's columns, 1-5 sources: forward, dx of
    every source, dW, db against the rounded float64 reference.  ReLU is back-propagated through the gate the kernel applied."""
    dev = _gpu()
    taps, bn, th, cins, cout, (H, W), bias, relu, res = case
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = conv_batch(case, cus)
    assert conv_tile(B, H, W, cout, cus) == (bn, th)
    print("bf16 conv<%d,%d,%d>: B=%d %dx%d sources %s -> %d, bias %d relu %d res %d" % (taps, bn, th, B, H, W, cins, cout, bias, relu, res))
    run_conv_case(dev, cins, cout, 3 if taps == 9 else 1, B, H, W, bias, relu, res, seed=taps * 1000 + bn + th)


# ------------------------------------------------------------------ 2. epilogue forms
@pytest.mark.parametrize("math", ["bf16", "bf16x6"])
@pytest.mark.parametrize("taps", [9, 1])
@pytest.mark.parametrize("res,relu,mask,acc", [
    (True, False, False, False), (False, True, True, False), (False, False, False, True), (True, True, False, True),
    (False, False, True, True), (True, True, True, False), (True, True, True, True), (False, True, False, False)])
def test_bf_epilogue_forms(math, taps, res, relu, mask, acc):
    """conv_raw in the bf16-plane kernels, every (residual, ReLU, mask, accumulate) form at ragged sizes:
    out = [mask > 0] relu(conv(r(x), r(w)) + b + residual) + previous; only the contraction is rounded (bf16), nothing is
    (bf16x6: against the unrounded float64 result, the mode's fp32-class bar)."""
    dev = _gpu()
    from bmc_hip import ops
    from bmc_hip.ops import ConvSpec, _packed_weight, _src, conv_raw, coutpad
    ops.set_math(math)
    g = torch.Generator().manual_seed(651 + 8 * res + 4 * relu + 2 * mask + acc + 16 * taps)
    if taps == 9:
        B, H, W, cin, Cn = 2, 19, 37, 128, 160
    else:
        B, H, W, cin, Cn = 3, 13, 21, 256, 80
    k = 3 if taps == 9 else 1
    x = torch.randn(B, H, W, cin, generator=g)
    w = torch.randn(Cn, cin, k, k, generator=g) / (cin * taps) ** 0.5
    b = torch.randn(Cn, generator=g)
    r = torch.randn(B, H, W, Cn, generator=g)
    m = torch.randn(B, H, W, Cn, generator=g)
    prev = torch.randn(B, H, W, Cn, generator=g)

    def ref(rounded):
        with O.operand_rounding("bf16" if rounded else None):
            y = O.conv2d(_nchw(x).double(), w.double(), b.double()).permute(0, 2, 3, 1)
        if res:
            y = y + r.double()
        if relu:
            y = torch.relu(y)
        if mask:
            y = torch.where(m.double() > 0, y, torch.zeros_like(y))
        return y + prev.double() if acc else y

    spec = ConvSpec.dense(cin)
    xg, bg, rg, mg = x.to(dev), b.to(dev), r.to(dev), m.to(dev)       # (referenced until the launch has run: lib.Src holds a raw pointer)
    out = prev.to(dev).clone()
    wp = _packed_weight(w.reshape(1, Cn, cin, taps).to(dev), spec, None)
    conv_raw([_src(xg, 0, cin, 0, None, 0, B)], wp, spec.kpad * taps * coutpad(Cn), bg, Cn, out.data_ptr(), H * W * Cn,
             Cn, B, H, W, Cn, taps, relu=relu, residual=_src(rg, 0, Cn, 0, None, 0, B) if res else None, bpg=B, accumulate=acc,
             mask=_src(mg, 0, Cn, 0, None, 0, B) if mask else None)
    torch.cuda.synchronize()
    print("%s taps=%d res=%d relu=%d mask=%d acc=%d" % (math, taps, res, relu, mask, acc))
    if math == "bf16":
        check("epilogue", out, ref(True), ref(False))
    else:
        check("epilogue (unrounded ref)", out, ref(False), bar=BAR_X6)


# ------------------------------------------------------------------ 3. batch views, weight groups, per-sample weights
@pytest.mark.parametrize("k,Cn", [(1, 16), (3, 48)])
@pytest.mark.parametrize("wgrad", [True, False])
def test_bf16_batch_views_and_groups(k, Cn, wgrad):
    """test_gpu_parity.py::test_conv_batch_views_and_groups in bf16: an operand shared by both halves of the doubled batch
    (mod = B), one rotated over it (shift = B, mod = 2B), two weight groups, a bias per group and a rotated residual.  With the
    weight frozen, the bias gradient of the grouped launch takes the column-sum route (ops.colsum) instead of the GEMM's."""
    dev = _gpu()
    B = 2
    run_conv_case(dev, [Cn, Cn], Cn, k, 2 * B, 9, 11, True, True, True, G=2, views=[(B, 0, B), (2 * B, B, 2 * B)],
                  res_view=(2 * B, 1, 2 * B), wgrad=wgrad, seed=5 + k)


def test_bf16_per_sample_weights_attention_apply():
    """G = B: one 128 x 128 weight matrix per sample plus a residual -- ops.attn_apply, the BIE's softmax(att) v in bf16 mode."""
    dev = _gpu()
    from bmc_hip import ops
    from bmc_hip.ops import View
    ops.set_math("bf16")
    g = torch.Generator().manual_seed(17)
    B, H, W, Cn = 3, 13, 19, 128
    p = torch.softmax(torch.randn(B, Cn, Cn, generator=g) * 3, -1)
    v = torch.randn(B, H, W, Cn, generator=g)
    r = torch.randn(B, H, W, Cn, generator=g)
    go = torch.randn(B, H, W, Cn, generator=g)
    pg, vg, rg = p.to(dev).requires_grad_(), v.to(dev).requires_grad_(), r.to(dev).requires_grad_()
    y = ops.attn_apply(pg, vg, residual=View(rg))
    y.backward(go.to(dev))
    torch.cuda.synchronize()
    refs = [conv_reference([(_nchw(v), 0, None)], p, None, (_nchw(r), 0, None), _nchw(go), None, B, B, rounded) for rounded in (True, False)]
    check("forward", _nchw(y), refs[0][0], refs[1][0])
    check("dv", _nchw(vg.grad), refs[0][1][0], refs[1][1][0])
    check("dP", pg.grad, refs[0][2], refs[1][2])
    check("residual gradient", _nchw(rg.grad), refs[0][4], bar=1e-12)


# ------------------------------------------------------------------ 4. weight gradient: both sides of the tap-row rule
@pytest.mark.parametrize("case", WGRAD_CASES, ids=["B%d_%dx%d_%dsrc_co%d_G%d" % (c[0], c[1], c[2], len(c[3]), c[4], c[5]) for c in WGRAD_CASES])
def test_bf16_weight_gradient_tap_row_rule(case, pgemm_log):
    """3x3 weight (+ bias) gradients through pgemm_bf_kernel<9,1>: the 64-column groups with one workgroup over all 9 taps
    (tap_groups = 1) and one tap row per workgroup (tap_groups = 3), partial 64-column / 128-row blocks (Cout 16, 48, 160),
    several sources, two weight groups -- dW and db (and the rest of the layer) against the rounded float64 reference."""
    dev = _gpu()
    B, H, W, cins, cout, G, tg = case
    run_conv_case(dev, cins, cout, 3, B, H, W, True, False, False, G=G, seed=B * 100 + H + cout)
    calls = [c for c in pgemm_log if c["taps"] == 9]
    print("    pgemm launches: %s" % calls)
    assert len(calls) == 1 and calls[0]["math"] == 1 and calls[0]["tap_groups"] == tg, calls


# ------------------------------------------------------------------ 5. merged weight gradients in both bf16 modes
class _WgradUse(torch.autograd.Function):
    """y = conv(view of x) + b through ops.conv; backward: the weight (+ bias) gradient only, through ops.wgrad_pgemm -- the
    route of the models' sink parameters, whose uses inside one window are queued and merged (pointer-table operands)."""

    @staticmethod
    def forward(ctx, x, w, b, B, shift, mod, spec):
        from bmc_hip import ops
        from bmc_hip.ops import View
        y = ops.conv([View(x, shift=shift, mod=mod)], w, b, spec, B=B, cache=False)
        ctx.save_for_backward(x)
        ctx.w, ctx.b, ctx.B, ctx.shift, ctx.mod, ctx.spec, ctx.window = w, b, B, shift, mod, spec, ops.current_window()
        return y

    @staticmethod
    def backward(ctx, gy):
        from bmc_hip import ops
        (x,) = ctx.saved_tensors
        g = gy.contiguous()
        B, H, W, Cout = g.shape
        taps = ctx.w.shape[-1] * ctx.w.shape[-2]
        a_src = ops._src(g, 0, Cout, 0, None, 0, B)
        x_src = ops._src(x, 0, x.shape[3], ctx.shift, ctx.mod, 0, B)
        dw, db = ops.wgrad_pgemm(a_src, [x_src], B, H, W, taps, Cout, ctx.spec, g.device, ctx.w, ctx.b, ctx.w.shape, keep=(g, x),
                                 window=ctx.window)
        return None, dw, db, None, None, None, None


# (images of the operand tensor, launch batch, shift, mod) of the 7 uses: batch sizes vary, use 4 rotates, use 6 shares
MERGE_USES = [(2, 2, 0, None), (1, 1, 0, None), (3, 3, 0, None), (4, 4, 1, 4), (2, 2, 0, None), (2, 4, 0, 2), (1, 1, 0, None)]


@pytest.mark.parametrize("math", ["bf16", "bf16x6"])
@pytest.mark.parametrize("k", [3, 1])
def test_merged_weight_gradients_in_bf16_modes(math, k, pgemm_log):
    """One contiguous leaf weight (a sink, ops.is_sink) used by 7 convolutions of one window: with WGRAD_MERGE = 5 the uses leave as
    one merged pixel-reduction launch of 5 and one of 2, reading their operands through pointer tables -- pgemm_bf_kernel<9,1,true>
    / <1,1,true> (bf16), pgemm_bf9x3_kernel<true> / pgemm_bf_kernel<1,3,true> (bf16x6).  .grad against the float64 sum over all
    uses (rounded for bf16, unrounded for bf16x6), and against the unmerged launches (WGRAD_MERGE = 1) to summation order."""
    dev = _gpu()
    from bmc_hip import ops
    from bmc_hip.ops import ConvSpec
    ops.set_math(math)
    g = torch.Generator().manual_seed(31 + k)
    H, W, cin, cout = 21, 27, 48, 80
    spec = ConvSpec.dense(cin)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g)
    xs = [torch.randn(n, H, W, cin, generator=g) for n, _, _, _ in MERGE_USES]
    gos = [torch.randn(nb, H, W, cout, generator=g) for _, nb, _, _ in MERGE_USES]

    def run(merge):
        old = ops.WGRAD_MERGE
        ops.WGRAD_MERGE = merge
        try:
            wg, bg = w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
            assert ops.is_sink(wg) and ops.is_sink(bg)
            ops.next_window()
            del pgemm_log[:]
            loss = 0
            for x, go, (_, nb, s, m) in zip(xs, gos, MERGE_USES):
                loss = loss + (_WgradUse.apply(x.to(dev), wg, bg, nb, s, m, spec) * go.to(dev)).sum()
            loss.backward()
            torch.cuda.synchronize()
            return wg.grad.clone(), bg.grad.clone(), list(pgemm_log)
        finally:
            ops.WGRAD_MERGE = old

    w5, b5, log5 = run(5)
    w1, b1, log1 = run(1)
    print("    merged launches: %s" % log5)
    tables = [c for c in log5 if c["table"]]
    assert len(tables) == 2 and sum(c["B"] for c in tables) == sum(u[1] for u in MERGE_USES), log5     # 5 uses + 2 uses
    assert all(c["math"] == ops.MATH_NAMES[math] for c in tables), log5
    assert len(log1) == 7 and not any(c["table"] for c in log1), log1

    def ref(rounded):
        wd, bd = w.double().requires_grad_(), b.double().requires_grad_()
        with O.operand_rounding("bf16" if rounded else None):
            for x, go, (n, nb, s, mod) in zip(xs, gos, MERGE_USES):
                xv = _nchw(x).double()[[(i + s) % (mod if mod is not None else nb) for i in range(nb)]]
                O.conv2d(xv, wd, bd).backward(_nchw(go).double())
        return wd.grad, bd.grad

    (wr, br), (wu, bu) = ref(True), ref(False)
    if math == "bf16":
        check("merged dW", w5, wr, wu)
        check("unmerged dW", w1, wr, wu)
    else:
        check("merged dW (unrounded ref)", w5, wu, bar=BAR_X6)
        check("unmerged dW (unrounded ref)", w1, wu, bar=BAR_X6)
    check("merged db", b5, br)
    check("merged vs unmerged dW", w5, w1, bar=BAR_MERGE)
    check("merged vs unmerged db", b5, b1, bar=BAR_MERGE)


# ------------------------------------------------------------------ 6. bf16-specific operands
def _ties(g, *shape):
    """Values exactly halfway between two bf16 neighbours, both parities: +-(1 + 2^-8) (rounds down to the even 1) and
    +-(1 + 3 2^-8) (rounds up to the even 1 + 2^-6), times 1 or 1/2.  The rounded operands' products and every partial sum of
    the launches below are exact in fp32, so any summation order gives the float64 value exactly."""
    m = torch.where(torch.rand(*shape, generator=g) < 0.5, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8)
    sgn = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (m * sgn * torch.exp2(-torch.randint(0, 2, shape, generator=g).float())).float()


@pytest.mark.parametrize("k", [3, 1])
def test_bf16_round_to_nearest_even_on_exact_ties(k):
    """Every operand is an exact tie: round-half-up or truncation would move each element by one bf16 ulp.  Forward, dx, dW, db
    equal the rounded float64 reference bit for bit (O.round_bf16 = RNE), and differ from the unrounded one."""
    dev = _gpu()
    from bmc_hip import ops
    from bmc_hip.ops import ConvSpec, View
    ops.set_math("bf16")
    g = torch.Generator().manual_seed(71 + k)
    B, H, W, cin, cout = 1, 9, 13, 32, 48
    x, w, go = _ties(g, B, H, W, cin), _ties(g, cout, cin, k, k), _ties(g, B, H, W, cout)
    b = torch.randint(-4, 5, (cout,), generator=g).float() * 0.25
    xg, wg, bg = x.to(dev).requires_grad_(), w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    y = ops.conv([View(xg)], wg, bg, ConvSpec.dense(cin))
    y.backward(go.to(dev))
    torch.cuda.synchronize()
    refs = [conv_reference([(_nchw(x), 0, None)], w, b, None, _nchw(go), None, 1, B, rounded) for rounded in (True, False)]
    for what, got, r, u in (("forward", _nchw(y), refs[0][0], refs[1][0]), ("dx", _nchw(xg.grad), refs[0][1][0], refs[1][1][0]),
                            ("dW", wg.grad, refs[0][2], refs[1][2]), ("db", bg.grad, refs[0][3], refs[1][3])):
        got = got.cpu()
        nbad = int((got != r.float()).sum())
        print("    %-8s elements off the RNE reference: %d of %d" % (what, nbad, got.numel()))
        assert nbad == 0, what
        if what != "db":
            assert not torch.equal(got, u.float()), what           # the ties really round


def _err_vs_scale(got, x, w, k, rounded):
    """max |got - ref| / sum |x| |w| over the outputs (ref, x, w rounded to bf16 or not), float64."""
    r = O.round_bf16 if rounded else (lambda t: t)
    xd, wd = r(_nchw(x).double().cpu()), r(w.double().cpu())
    ref = F.conv2d(xd, wd, None, padding=k // 2)
    scale = F.conv2d(xd.abs(), wd.abs(), None, padding=k // 2)
    return ((_nchw(got).double().cpu() - ref).abs() / scale.clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("k", [3, 1])
def test_bf16_wide_dynamic_range(k):
    """Magnitudes over 2^-40 .. 2^40 in both operands (products over 2^-80 .. 2^80): the error against the rounded reference,
    measured against sum |r(x)| |r(w)| (the scale of any fp32 summation error), is fp32-accumulation class at every exponent."""
    dev = _gpu()
    from bmc_hip import ops
    from bmc_hip.ops import ConvSpec, View
    ops.set_math("bf16")
    g = torch.Generator().manual_seed(81 + k)
    B, H, W, Cn = 2, 24, 40, 128
    mant = lambda *s: (1.0 + torch.rand(*s, generator=g)) * (torch.randint(0, 2, s, generator=g) * 2 - 1)
    x = (mant(B, H, W, Cn) * torch.exp2(torch.randint(-40, 41, (B, H, W, Cn), generator=g).float())).to(dev)
    w = (mant(Cn, Cn, k, k) * torch.exp2(torch.randint(-40, 41, (Cn, Cn, k, k), generator=g).float())).to(dev)
    with torch.no_grad():
        y = ops.conv([View(x)], w, None, ConvSpec.dense(Cn))
    er, eu = _err_vs_scale(y, x, w, k, True), _err_vs_scale(y, x, w, k, False)
    print("wide range k=%d: max |err| / sum|r(x)||r(w)|: %.2e vs rounded, %.2e vs unrounded" % (k, er, eu))
    assert torch.isfinite(y).all()
    assert er < BAR_WIDE and eu >= RESOLUTION * er, (er, eu)


def test_bf16_denormals_and_nonfinite_semantics():
    """Exceptional values in the one-plane mode, as the MI355X treats them:
      * subnormal fp32 activations round to subnormal bf16, and neither the conversion (v_cvt_pk_bf16_f32) nor the bf16 matrix
        core flushes them: outputs over purely subnormal windows (~1e-41) keep them, within K * 2^-150 (one fp32 rounding per
        product in the subnormal range; measured 7.0e-46 against outputs of 9.7e-42) of the rounded float64 reference --
        far inside K * 2^-126 * max|w|, what flushing them would cost; windows of normal operands keep the mode's error;
      * outputs that touch an Inf operand are non-finite, outputs that touch a NaN are NaN, all others are finite and unaffected."""
    dev = _gpu()
    from bmc_hip import ops
    from bmc_hip.ops import ConvSpec, View
    ops.set_math("bf16")
    g = torch.Generator().manual_seed(9)
    B, H, W, Cn, k = 1, 16, 32, 128, 3
    x = torch.randn(B, H, W, Cn, generator=g)
    x[:, :, :16] *= 1e-41                     # left half of the image: subnormal activations
    w = torch.randn(Cn, Cn, k, k, generator=g) / 34.0
    x, w = x.to(dev), w.to(dev)
    with torch.no_grad():
        y = ops.conv([View(x)], w, None, ConvSpec.dense(Cn))
    xr, wr = O.round_bf16(_nchw(x).double().cpu()), O.round_bf16(w.double().cpu())
    ref = F.conv2d(xr, wr, None, padding=1)
    aerr = (_nchw(y).double().cpu() - ref).abs()
    bound = Cn * k * k * 2.0 ** -126 * w.abs().max().item()
    sub = aerr[:, :, :, :14]
    print("subnormal windows: max |y| %.2e, max |ref| %.2e, max |err| %.2e (bound %.2e): subnormals %s" % (
        _nchw(y)[:, :, :, :14].abs().max().item(), ref[:, :, :, :14].abs().max().item(), sub.max().item(), bound,
        "flushed" if _nchw(y)[:, :, :, :14].abs().max().item() == 0 else "kept"))
    assert sub.max().item() <= bound, (sub.max().item(), bound)
    kept = Cn * k * k * 2.0 ** -150
    assert _nchw(y)[:, :, :, :14].abs().max().item() > 0 and sub.max().item() <= kept, (sub.max().item(), kept)
    scale = F.conv2d(xr.abs(), wr.abs(), None, padding=1)
    assert (aerr[:, :, :, 18:] / scale[:, :, :, 18:]).max().item() < 1e-6
    # non-finite operands
    x2 = torch.randn(B, H, W, Cn, generator=g).to(dev)
    x2[0, 3, 5, 7] = float("inf")
    x2[0, 10, 20, 9] = float("nan")
    with torch.no_grad():
        y2 = ops.conv([View(x2)], w, None, ConvSpec.dense(Cn))[0].cpu()
    t_inf = torch.zeros(H, W, dtype=torch.bool)
    t_inf[2:5, 4:7] = True
    t_nan = torch.zeros(H, W, dtype=torch.bool)
    t_nan[9:12, 19:22] = True
    assert (~torch.isfinite(y2[t_inf])).all() and torch.isnan(y2[t_nan]).all()
    untouched = ~(t_inf | t_nan)
    assert torch.isfinite(y2[untouched]).all()
    x2f = x2.clone()
    x2f[0, 3, 5, 7] = 0.0
    x2f[0, 10, 20, 9] = 0.0
    ref2 = F.conv2d(O.round_bf16(_nchw(x2f).double().cpu()), wr, None, padding=1)[0].permute(1, 2, 0)
    assert rel_l2(y2[untouched], ref2[untouched]) < BAR
