"""ops.wgrad, the one weight-gradient executor, each route of ops.wgrad_route once against float64 F.conv2d gradients computed on
the CPU, into both destinations: returned to autograd (a non-leaf weight) and accumulated into .grad (a leaf, called twice
and compared with twice the gradient).

Bars, each from the existing test of the kernel the route ends in: the F(2x2) Winograd weight gradient rel-L2 2e-6
(tests/test_gpu_r3.py::test_winograd_weight_gradient_vs_float64), the F(4x4) one element-wise 2e-5 / rel-L2 1e-5 / bias 2e-6
(tests/test_gpu_wgrad4.py), the pixel-reduction GEMM rel-L2 3e-5 (tests/test_gpu_pgemm9_wavemap.py)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bmcnet-esr_amd"))

pytestmark = pytest.mark.gpu
BAR_WINO, BAR_PGEMM = 2e-6, 3e-5
BAR_WINO4_MAX, BAR_WINO4_REL, BAR_WINO4_BIAS_MAX = 2e-5, 1e-5, 2e-6


@pytest.fixture
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmc_hip import ops as o
    old = o.MATH, o.WGRAD_MERGE, o.PROFILE
    o.set_math("fp32")
    o.set_accumulate_param_grads(True)
    yield o
    o.MATH, o.WGRAD_MERGE, o.PROFILE = old


def _reference(xs, g, taps):
    """float64 (dW [Cout, sum Cin, k, k], db [Cout]) of a 'same' convolution over the concatenated NHWC sources."""
    x64 = torch.cat([x.detach().cpu() for x in xs], 3).double().permute(0, 3, 1, 2)
    g64 = g.detach().cpu().double().permute(0, 3, 1, 2)
    k = 3 if taps == 9 else 1
    w = torch.zeros(g.shape[3], x64.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(g.shape[3], dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, w, b, padding=k // 2).backward(g64)
    return w.grad, b.grad


def _rel(a, ref):
    return float((a.detach().cpu().double() - ref).norm() / ref.norm())


def _max_err(a, ref):
    return float((a.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _profiled(ops, fn):
    ops.PROFILE = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None


def _both_destinations(ops, widths, Cout, taps, B, H, W, route, kinds, check, seed, nonleaf_route=None):
    """One use of a convolution with these source widths through ops.wgrad; check(dW, db, ref_w, ref_b, factor) holds the bars."""
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    xs = [torch.randn(B, H, W, n, device=dev) for n in widths]
    g = torch.randn(B, H, W, Cout, device=dev)
    ref_w, ref_b = _reference(xs, g, taps)
    spec = ops.ConvSpec.dense(*widths)
    metas = [ops.View(x).meta() for x in xs]
    a_src, srcs = ops._src(g, 0, Cout, 0, None, 0, B), [ops._src(x, *m, B) for x, m in zip(xs, metas)]
    k = 3 if taps == 9 else 1
    run = lambda w, b: ops.wgrad(a_src, srcs, spec, B, H, W, taps, Cout, dev, w, b, keep=(g, *xs), metas=metas, merge_pgemm=True)
    # returned to autograd: a non-leaf weight
    w = torch.zeros(Cout, sum(widths), k, k, device=dev, requires_grad=True) * 1.0
    b = torch.zeros(Cout, device=dev, requires_grad=True) * 1.0
    assert ops.wgrad_route(spec, a_src, srcs, metas, taps, Cout, 1, w, b, True)[0] == (nonleaf_route or route)
    dw, db = run(w, b)
    check(dw, db, ref_w, ref_b, 1, nonleaf_route or route)
    # accumulated into .grad: a leaf, twice
    w, b = torch.nn.Parameter(w.detach()), torch.nn.Parameter(b.detach())
    assert ops.wgrad_route(spec, a_src, srcs, metas, taps, Cout, 1, w, b, True)[0] == route
    out, seen = _profiled(ops, lambda: run(w, b))
    assert out == (None, None) and seen == kinds, seen
    assert run(w, b) == (None, None)
    check(w.grad, b.grad, ref_w, ref_b, 2, route)


def _bars_by_columns(wino_cols):
    """The Winograd bar on the weight columns a Winograd launch wrote and on its bias, the pixel-reduction bar on the rest."""
    def check(dw, db, ref_w, ref_b, factor, route):
        cols = wino_cols if route != "pgemm" else []
        mask = torch.zeros(ref_w.shape[1], dtype=torch.bool)
        for c0 in cols:
            mask[c0:c0 + 128] = True
        if mask.any():
            assert _rel(dw[:, mask], factor * ref_w[:, mask]) < BAR_WINO
        if not mask.all():
            assert _rel(dw[:, ~mask], factor * ref_w[:, ~mask]) < BAR_PGEMM
        assert _rel(db, factor * ref_b) < (BAR_WINO if cols else BAR_PGEMM)
    return check


def test_wino_route_f2x2(ops):
    _both_destinations(ops, [128], 128, 9, 2, 24, 32, "wino", ["wgrad_wino<9>"], _bars_by_columns([0]), 1)


@pytest.mark.parametrize("H,kind", [(96, "wgrad_wino4<9>"), (92, "wgrad_wino<9>")])
def test_wino_route_f4x4_threshold_both_sides(ops, H, kind):
    """batch 8 at 96x64 is exactly 768 stages, the F(4x4) threshold; at 92x64 (736 stages) F(2x2) keeps the launch."""
    B, W = 8, 64
    assert ops.WINO4_WGRAD and ops.wgrad_wino4_ok(B, H, W) == (H == 96)
    assert B * ((H + 3) // 4) * (((W + 3) // 4 + 3) // 4) == (768 if H == 96 else 736)

    def f4(dw, db, ref_w, ref_b, factor, route):
        assert _max_err(dw, factor * ref_w) < BAR_WINO4_MAX and _rel(dw, factor * ref_w) < BAR_WINO4_REL
        assert _max_err(db, factor * ref_b) < BAR_WINO4_BIAS_MAX
    _both_destinations(ops, [128], 128, 9, B, H, W, "wino", [kind], f4 if H == 96 else _bars_by_columns([0]), H)


def test_split_route(ops):
    """128 + 16 sources: the wide one through the Winograd kernel (with the bias), the narrow one through the pixel-reduction GEMM,
    both into one .grad; a non-leaf weight keeps the one pixel-reduction launch."""
    _both_destinations(ops, [128, 16], 128, 9, 2, 24, 32, "split", ["wgrad_wino<9>", "pgemm_kernel<9>"], _bars_by_columns([0]), 3,
                       nonleaf_route="pgemm")


def test_pgemm_route_3x3_tap_rows(ops):
    _both_destinations(ops, [48], 48, 9, 1, 13, 21, "pgemm", ["pgemm_kernel<9>"], _bars_by_columns([]), 4)


def test_pgemm_route_1x1(ops):
    _both_destinations(ops, [128], 128, 1, 2, 24, 32, "pgemm", ["pgemm_kernel<1>"], _bars_by_columns([]), 5)


def test_wino_groups_route_through_conv_groups(ops):
    """conv_groups with two parameters: one Winograd weight gradient per group on the group's batch window; ConvFn re-stacks what
    comes back for non-leaf parameters."""
    dev = torch.device("cuda:0")
    torch.manual_seed(6)
    B, H, W, G = 4, 24, 32, 2
    x = torch.randn(B, H, W, 128, device=dev)
    g = torch.randn(B, H, W, 128, device=dev)
    spec = ops.ConvSpec.dense(128)
    refs = [_reference([x[i * 2:i * 2 + 2]], g[i * 2:i * 2 + 2], 9) for i in range(G)]
    leaves_w = [torch.nn.Parameter(torch.randn(128, 128, 3, 3, device=dev) * 0.02) for _ in range(G)]
    leaves_b = [torch.nn.Parameter(torch.zeros(128, device=dev)) for _ in range(G)]
    for derive, passes in ((lambda p: p, 2), (lambda p: p * 1.0, 1)):           # into .grad (twice) / back to autograd
        for p in leaves_w + leaves_b:
            p.grad = None
        for _ in range(passes):
            ops.next_window()
            ws, bs = tuple(derive(p) for p in leaves_w), tuple(derive(p) for p in leaves_b)
            y = ops.conv_groups([ops.View(x)], ws, bs, spec)
            _, seen = _profiled(ops, lambda: (y * g).sum().backward())
            assert [k for k in seen if "wgrad" in k or "pgemm" in k] == ["wgrad_wino<9>"] * G, seen
        for i in range(G):
            assert _rel(leaves_w[i].grad, passes * refs[i][0]) < BAR_WINO and _rel(leaves_b[i].grad, passes * refs[i][1]) < BAR_WINO


def test_five_uses_of_one_leaf_weight_leave_as_one_merged_launch(ops):
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    B, H, W, uses = 2, 24, 32, 5
    ops.WGRAD_MERGE = uses
    spec = ops.ConvSpec.dense(128)
    w = torch.nn.Parameter(torch.randn(128, 128, 3, 3, device=dev) * 0.02)
    b = torch.nn.Parameter(torch.zeros(128, device=dev))
    xs = [torch.randn(B, H, W, 128, device=dev) for _ in range(uses)]
    gs = [torch.randn(B, H, W, 128, device=dev) for _ in range(uses)]
    ops.next_window()
    loss = sum((ops.conv([ops.View(x)], w, b, spec) * g).sum() for x, g in zip(xs, gs))
    _, seen = _profiled(ops, loss.backward)
    assert [k for k in seen if "wgrad" in k or "pgemm" in k] == ["wgrad_wino<9>"], seen
    refs = [_reference([x], g, 9) for x, g in zip(xs, gs)]
    assert _rel(w.grad, sum(r[0] for r in refs)) < BAR_WINO and _rel(b.grad, sum(r[1] for r in refs)) < BAR_WINO
