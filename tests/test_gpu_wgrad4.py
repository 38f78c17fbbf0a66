"""The F(4x4) Winograd weight gradient (csrc/wino4_wgrad.hip) as the default for large frames: multi-stage workgroups whose stage
ranges cross tile rows and images, the reduction at every split count and output form, both sides of the dispatch threshold, and
its place in the C2 training step."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _stages(B, H, W):
    return B * ((H + 3) // 4) * (((W + 3) // 4 + 3) // 4)


def _launch(ops, g, x, nsplit, bias):
    """bmc_wgrad_wino4 on NHWC operands -> (partial sums, bias partials or None)."""
    from bmc_hip import lib
    B, H, W, _ = x.shape
    a_src, x_src = ops._src(g, 0, 128, 0, None, 0, B), ops._src(x, 0, 128, 0, None, 0, B)
    part = torch.full((nsplit * 36 * 128 * 128,), float("nan"), device=x.device)
    bpart = torch.full((nsplit * 128,), float("nan"), device=x.device) if bias else None
    lib.call(lib._ww4, "bmc_wgrad_wino4", C.byref(a_src), C.byref(x_src), B, H, W, nsplit, part.data_ptr(),
             bpart.data_ptr() if bias else None, ops._stream())
    return part, bpart


def _reduce(ops, part, nsplit, dw, k0, accumulate, bpart=None, db=None):
    from bmc_hip import lib
    lib.call(lib._ww4_red, "bmc_wgrad_wino4_reduce", part.data_ptr(), nsplit, dw.data_ptr(), dw.shape[1], k0, int(accumulate),
             bpart.data_ptr() if bpart is not None else None, db.data_ptr() if db is not None else None, ops._stream())


def _max_err(a, ref):
    """element-wise: the worst |a - ref| over the largest |ref| (a race on a few taps shows here, not in a rel-L2)"""
    return float((a.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _rel(a, ref):
    return float((a.detach().cpu().double() - ref).norm() / ref.norm())


@pytest.mark.parametrize("B,H,W", [
    (3, 37, 70),          # 150 stages over 32 splits: 4-5 per workgroup, ranges across tile rows (5 stages each) and images
    (2, 90, 118),         # 368 stages: 11-12 per workgroup, ragged last stage of every row (30 tiles = 7.5 stages)
    (6, 21, 46),          # ragged in both axes, rows of 3 stages: 108 stages, 3-4 per workgroup, every one across a row
])
def test_multi_stage_workgroups_elementwise_vs_float64_and_bit_identical(B, H, W):
    dev = _gpu()
    from bmc_hip import lib, ops
    from test_gpu_r3 import _wgrad_reference
    nsplit = lib._ww4_nsplit(B, H, W)
    assert _stages(B, H, W) >= 3 * nsplit
    torch.manual_seed(B * 7 + H + W)
    x = torch.randn(B, H, W, 128, device=dev)
    g = torch.randn(B, H, W, 128, device=dev)
    ref_w, ref_b = _wgrad_reference(x, g)
    outs = []
    for _ in range(2):
        part, bpart = _launch(ops, g, x, nsplit, True)
        dw = torch.full((128, 128, 3, 3), float("nan"), device=dev)
        db = torch.full((128,), float("nan"), device=dev)
        _reduce(ops, part, nsplit, dw, 0, False, bpart, db)
        torch.cuda.synchronize()
        outs.append((dw, db))
    (dw, db), (dw2, db2) = outs
    print("B%d %dx%d nsplit %d: dW max %.2e rel-L2 %.2e, db max %.2e" % (B, H, W, nsplit, _max_err(dw, ref_w), _rel(dw, ref_w),
                                                                         _max_err(db, ref_b)))
    assert _max_err(dw, ref_w) < 2e-5 and _rel(dw, ref_w) < 1e-5
    assert _max_err(db, ref_b) < 2e-6
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("nsplit", [1, 3, 7, 13, 24, "max"])
def test_reduction_split_counts_bias_accumulate_and_column_windows(nsplit):
    """The same operands through every reduction form: split counts of 1, odd, not a multiple of 8 and the largest the launch
    allows; with and without bias; overwriting and accumulating; the column windows k0 = 0 / 80 / 160 of a 288-column weight."""
    dev = _gpu()
    from bmc_hip import lib, ops
    from test_gpu_r3 import _wgrad_reference
    B, H, W = 2, 30, 61
    if nsplit == "max":
        nsplit = lib._ww4_nsplit(B, H, W)
    assert nsplit <= _stages(B, H, W)
    torch.manual_seed(400 + nsplit)
    x = torch.randn(B, H, W, 128, device=dev)
    g = torch.randn(B, H, W, 128, device=dev)
    ref_w, ref_b = _wgrad_reference(x, g)
    part, bpart = _launch(ops, g, x, nsplit, True)
    part_nb, _ = _launch(ops, g, x, nsplit, False)
    torch.cuda.synchronize()
    assert torch.equal(part, part_nb)
    for k0 in (0, 80, 160):
        base = torch.randn(128, 288, 3, 3, device=dev)
        dbase = torch.randn(128, device=dev)
        for acc in (False, True):
            for bias in (False, True):
                dw, db = base.clone(), dbase.clone()
                _reduce(ops, part, nsplit, dw, k0, acc, bpart if bias else None, db if bias else None)
                torch.cuda.synchronize()
                win = dw[:, k0:k0 + 128]
                want = ref_w + (base[:, k0:k0 + 128].cpu().double() if acc else 0)
                assert _max_err(win, want) < 2e-5, (k0, acc, bias)
                outside = torch.cat([dw[:, :k0], dw[:, k0 + 128:]], 1)
                assert torch.equal(outside, torch.cat([base[:, :k0], base[:, k0 + 128:]], 1))
                if bias:
                    want_b = ref_b + (dbase.cpu().double() if acc else 0)
                    assert _max_err(db, want_b) < 2e-6
                else:
                    assert torch.equal(db, dbase)


@pytest.mark.parametrize("B,H,W", [
    (4, 72, 96),          # 432 stages = 13.5 per workgroup: F(2x2)
    (7, 60, 104),         # 7 x 15 x 7 = 735 stages = 23.0 per workgroup: F(2x2), just below
    (8, 60, 104),         # 840 stages = 26.3 per workgroup: F(4x4), just above
    (8, 72, 96),          # 864 stages = 27 per workgroup: F(4x4)
])
def test_dispatch_threshold_both_sides_vs_float64(B, H, W):
    dev = _gpu()
    from bmc_hip import ops
    from test_gpu_r3 import _wgrad_reference
    assert ops.WINO4_WGRAD and ops.WINO4_WGRAD_MIN_STAGES == 24
    f4 = ops.wgrad_wino4_ok(B, H, W)
    assert f4 == (_stages(B, H, W) >= 32 * 24)
    torch.manual_seed(B + H + W)
    x = torch.randn(B, H, W, 128, device=dev)
    g = torch.randn(B, H, W, 128, device=dev)
    spec = ops.ConvSpec.dense(128)
    w = torch.zeros(128, 128, 3, 3, device=dev)
    b = torch.zeros(128, device=dev)
    ops.PROFILE = []
    try:
        dw, db = ops._wgrad_plain(g, x, spec, w, b, 9)
        torch.cuda.synchronize()
        kinds = {r[0] for r in ops.PROFILE}
    finally:
        ops.PROFILE = None
    assert kinds == {"wgrad_wino4<9>" if f4 else "wgrad_wino<9>"}, kinds
    ref_w, ref_b = _wgrad_reference(x, g)
    assert _max_err(dw, ref_w) < 2e-5 and _rel(dw, ref_w) < 1e-5
    assert _max_err(db, ref_b) < 2e-6


def test_thresholds_keep_the_side_stream_test_on_f2x2():
    """test_gpu_r4's side-stream test needs 4-image 72x96 launches on F(2x2); the 8-image C2 launches must take F(4x4)."""
    from bmc_hip import ops
    assert not ops.wgrad_wino4_ok(4, 72, 96)
    assert ops.wgrad_wino4_ok(8, 180, 240) and ops.wgrad_wino4_ok(16, 180, 240)


def test_c2_steady_state_backward_issues_f4x4_weight_gradients():
    """The bench's C2 shape (BMCNet x4, 128 channels, 180x240, batch 4): from the second step on, the dense 3x3 weight gradients
    of the full-size launches run on the F(4x4) kernel."""
    dev = _gpu()
    from bmc_hip import ops
    from models.BMCNet import BMCNet
    from train_step import bptt_step
    ops.set_math("fp32")
    scale, n_c, n_b, B, L, H, W = 4, 128, 1, 4, 3, 180, 240
    gen = torch.Generator().manual_seed(77)
    inp = torch.poisson(torch.full((B, L, 2, H, W), 0.5), generator=gen).to(dev)
    gt = torch.poisson(torch.full((B, L, 2, scale * H, scale * W), 0.5), generator=gen).to(dev)
    torch.manual_seed(78)
    m = BMCNet(scale, n_c, n_b).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    bptt_step(m, opt, inp, gt, n_c, scale)
    ops.PROFILE = []
    try:
        loss, _ = bptt_step(m, opt, inp, gt, n_c, scale)
        torch.cuda.synchronize()
        kinds = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert torch.isfinite(torch.as_tensor(float(loss)))
    n4 = kinds.count("wgrad_wino4<9>")
    print("C2 step: %d wgrad_wino4<9>, %d wgrad_wino<9> launches" % (n4, kinds.count("wgrad_wino<9>")))
    assert n4 > 0, sorted(set(kinds))
