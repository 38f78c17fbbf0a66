"""Batch segments on convolution operands (-m gpu): one launch whose images come from two tensors (ops.View(t, t2=, seg=),
bmc_conv_args_t::seg_b), and the node built on it (ops.ResPairFn: the two residual blocks of a ParallelBlk as one launch per layer).

The bar is bit identity and needs no tolerance: a workgroup tile lies inside one image, and the same kernel computes it from the
same packed weights in the same order wherever the image's base pointer comes from."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: E402,F401

CN = 128
H, W = 35, 51       # not multiples of 4 (nor of the F(2x2) kernel's 8 x 16 tile): ragged tiles on both edges


def _wg_tiles(wino, B):
    """Workgroup tiles of a forced-route launch of B images of H x W: F(4x4) 16 tiles of 4x4 pixels, F(2x2) 8 (or 4) x 16 pixels."""
    from bmc_hip import ops
    if wino == 4:
        return B * ((((H + 3) // 4) * ((W + 3) // 4) + 15) // 16)
    return ops.wino_tiles(B, H, W, CN)[0]


def _carve(n_first, n_second, second_below, dev, gen):
    """Two [n, H, W, CN] tensors out of one allocation, one image apart, the second below or above the first: the sign of the
    segment's delta is the test's choice, not the allocator's."""
    pool = torch.randn(n_first + n_second + 1, H, W, CN, generator=gen, device=dev)
    if second_below:
        return pool[n_second + 1:], pool[:n_second]
    return pool[:n_first], pool[n_first + 1:]


@pytest.fixture(scope="module")
def weights():
    dev = _gpu()
    g = torch.Generator(device=dev).manual_seed(7)
    return (torch.randn(2, CN, CN, 9, generator=g, device=dev) * 0.03, torch.randn(2, CN, generator=g, device=dev) * 0.3)


CASES = [
    # (route, groups, images, split, epilogue)
    (4, 2, 40, 20, "relu"), (4, 2, 40, 20, "res"), (4, 1, 40, 17, "mask"), (4, 2, 40, 17, "res+relu"), (4, 2, 4, 2, "res"),
    (2, 2, 40, 20, "relu"), (2, 2, 40, 20, "res"), (2, 1, 40, 17, "mask"), (2, 2, 40, 17, "res+relu"), (2, 2, 4, 2, "res"),
]


@pytest.mark.parametrize("wino,G,B,seg,epi", CASES)
def test_segmented_launch_equals_launch_over_cat(weights, wino, G, B, seg, epi):
    """A launch over [x1[:seg] | x2[:B - seg]] read in place == the same launch over torch.cat of the two.  40 images of 35x51 are
    320 F(4x4) workgroup tiles (8 per image, the last one ragged: 117 = 7 * 16 + 5 Winograd tiles) and 800 (8-row) F(2x2) ones:
    more than the device has CUs, so workgroups walk across the split and the XCD map is active; 4 images stay below one round.
    The source's second tensor lies BELOW its first (negative delta), the epilogue operand's above."""
    from bmc_hip import ops
    from bmc_hip.ops import ConvSpec, _packed_weight, _src, conv_raw, coutpad
    dev = _gpu()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    ntiles = _wg_tiles(wino, B)
    print("workgroup tiles %d, CUs %d" % (ntiles, cus))
    assert (ntiles > cus) if B == 40 else (ntiles < cus)
    g = torch.Generator(device=dev).manual_seed(100 * wino + B + seg)
    x1, x2 = _carve(seg, B - seg, True, dev, g)
    e1, e2 = _carve(seg, B - seg, False, dev, g)
    w, bias = weights
    spec = ConvSpec.dense(CN)
    wp = _packed_weight(w[:G].contiguous(), spec, None, wino=wino)
    xs = _src(x1, 0, CN, 0, None, 0, B, x2, seg)
    es = _src(e1, 0, CN, 0, None, 0, B, e2, seg)
    assert xs.seg_b == seg and xs.seg_delta < 0 < es.seg_delta
    xc, ec = torch.cat([x1[:seg], x2[:B - seg]]), torch.cat([e1[:seg], e2[:B - seg]])
    use_mask, use_res, relu = epi == "mask", epi.startswith("res"), epi.endswith("relu")

    def run(src, esrc):
        out = torch.full((B, H, W, CN), 0.25, device=dev)
        conv_raw([src], wp, spec.kpad * 9 * coutpad(CN), None if use_mask else bias[:G].contiguous(), 0 if use_mask else CN, out.data_ptr(),
                 H * W * CN, CN, B, H, W, CN, 9, relu=relu, residual=esrc if use_res else None, bpg=B // G,
                 mask=esrc if use_mask else None, wino=wino)
        return out

    got = run(xs, es)
    ref = run(_src(xc, 0, CN, 0, None, 0, B), _src(ec, 0, CN, 0, None, 0, B))
    assert torch.equal(got, ref)
    assert float(ref.abs().max()) > 0.5          # (a launch happened)
    if use_mask:
        assert 0.3 < float((ref == 0).float().mean()) < 0.7


def _conv_args(B, src, out, wp, math, residual=None):
    from bmc_hip import lib
    from bmc_hip.ops import _null_src, coutpad
    a = lib.ConvArgs()
    a.nsrc = 1
    a.src[0] = src
    a.wpacked = wp.data_ptr()
    a.w_group_stride = 0
    a.batch_per_group = B
    a.out, a.out_batch_stride, a.out_pix_stride = out.data_ptr(), H * W * CN, CN
    a.B, a.H, a.W, a.Cout, a.Coutpad, a.taps = B, H, W, CN, coutpad(CN), 9
    a.residual = residual if residual is not None else _null_src()
    a.mask = _null_src()
    a.math = math
    return a


def test_segments_are_refused_where_they_are_not_served(weights):
    """The direct and the bf16-plane kernels know no segment; seg_b = 0 or B with a delta, a delta on an absent operand and a
    batch shift beside a segment are malformed: bmc_conv returns the error before any launch (the output keeps its fill)."""
    import ctypes as C
    from bmc_hip import lib
    from bmc_hip.ops import ConvSpec, _packed_weight, _src, _stream
    dev = _gpu()
    B, seg = 4, 2
    g = torch.Generator(device=dev).manual_seed(3)
    x1, x2 = _carve(seg, B - seg, True, dev, g)
    w, _ = weights
    spec = ConvSpec.dense(CN)
    out = torch.full((B, H, W, CN), 0.25, device=dev)
    xs = _src(x1, 0, CN, 0, None, 0, B, x2, seg)

    def refused(a, what):
        with pytest.raises(RuntimeError, match=what):
            lib.call(lib._conv, "bmc_conv", C.byref(a), _stream())

    wp_direct = _packed_weight(w[:1].contiguous(), spec, None)
    wp4 = _packed_weight(w[:1].contiguous(), spec, None, wino=4)
    for math in (0, 1, 3):                                     # direct fp32, bf16, bf16x6
        a = _conv_args(B, xs, out, wp_direct, math)
        a.seg_b, a.src_seg_delta[0] = seg, xs.seg_delta
        refused(a, "Winograd kernels only")
    for math in (4, 5):
        for bad in (0, B, -1, B + 3):                          # split point outside [1, B)
            a = _conv_args(B, xs, out, wp4, math)
            a.seg_b, a.src_seg_delta[0] = bad, xs.seg_delta
            refused(a, "seg_b")
        a = _conv_args(B, xs, out, wp4, math)                  # a batch shift beside the segment
        a.seg_b, a.src_seg_delta[0] = seg, xs.seg_delta
        a.src[0].batch_shift = 1
        refused(a, "batch shift")
        a = _conv_args(B, xs, out, wp4, math)                  # a wrapping modulus beside the segment
        a.seg_b, a.src_seg_delta[0] = seg, xs.seg_delta
        a.src[0].batch_mod = seg
        refused(a, "batch shift")
        a = _conv_args(B, xs, out, wp4, math)                  # a delta on an operand the launch does not have
        a.seg_b, a.residual_seg_delta = seg, 64
        refused(a, "absent operand")
        a = _conv_args(B, xs, out, wp4, math)
        a.seg_b, a.src_seg_delta[1] = seg, 64
        refused(a, "absent operand")
        a = _conv_args(B, xs, out, wp4, math)                  # a second tensor that is not 16-byte aligned
        a.seg_b, a.src_seg_delta[0] = seg, xs.seg_delta + 1
        refused(a, "16-byte")
    torch.cuda.synchronize()
    assert bool((out == 0.25).all())
    # the host side refuses a segmented operand for every other entry point
    from bmc_hip import ops
    with pytest.raises(ValueError, match="convolution launches only"):
        ops.pgemm_raw(xs, [xs], B, H, W, 9, B, CN, CN, dev)


def _blocks(dev, zero_bias):
    from models.submodules import ResidualBlock_noBN
    torch.manual_seed(11)
    blks = [ResidualBlock_noBN(CN).to(dev) for _ in range(2)]
    with torch.no_grad():
        for blk in blks:
            for conv in (blk.conv1, blk.conv2):
                conv.weight.mul_(5.0)
                if zero_bias:
                    conv.bias.zero_()
                else:       # dense: every element well away from zero (ops.bias_dense), both signs
                    conv.bias.copy_((0.01 + 0.1 * torch.rand(CN, device=dev)) * torch.where(torch.rand(CN, device=dev) < 0.5, -1.0, 1.0))
    return blks


def _params(blk):
    return (blk.conv1.weight, blk.conv1.bias, blk.conv2.weight, blk.conv2.bias)


def _run_node(paired, blks, xa, xb, gy, grad):
    from bmc_hip import bie, ops
    names = [n for n, _ in blks[0].named_parameters()]
    for blk in blks:
        for p in blk.parameters():
            p.grad = None
    xa = xa.clone().requires_grad_(grad)
    xb = xb.clone().requires_grad_(grad)
    B2 = xa.shape[0]
    with (torch.enable_grad() if grad else torch.no_grad()):
        if paired:
            y = ops.res_pair(xa, xb, _params(blks[0]), _params(blks[1]), blks[0]._spec)
        else:       # the two nodes the pair replaces, as models/BMCNet.py built them
            slot = ops.OutSlot(torch.empty((2 * B2,) + tuple(xa.shape[1:]), device=xa.device), 0)
            a = blks[0].forward_nhwc(xa, out=slot)
            b = blks[1].forward_nhwc(xb, out=ops.OutSlot(slot.t, B2))
            y = bie.Stack2Fn.apply(a, b, slot) if grad else slot.t
        out = {"y": y.detach().clone()}
        if grad:
            y.backward(gy)
            ops.wgrad_join()
            torch.cuda.synchronize()
            out["dxa"], out["dxb"] = xa.grad.clone(), xb.grad.clone()
            for i, blk in enumerate(blks):
                for n, p in blk.named_parameters():
                    out["%d.%s" % (i, n)] = p.grad.clone()
            assert len(out) == 3 + 2 * len(names) == 11
    return out


@pytest.mark.parametrize("route,bias", [(4, "dense"), (2, "zero"), (2, "dense")])
@pytest.mark.parametrize("grad", [True, False])
def test_res_pair_node_equals_two_res_block_nodes(monkeypatch, route, bias, grad):
    """ops.ResPairFn against the two ResBlockFn nodes + Stack2Fn it replaces at 36x52, B2 = 4, 128 channels: the output, both
    input gradients, the four weight and the four bias gradients, torch.equal; also under no_grad.  The thresholds are lowered
    HERE so that one block's 4 images take the F(4x4) kernel (dense biases), or the F(2x2) kernel (F(4x4) switched off): with
    zero biases the pair shares its launches there, with non-zero ones it must keep a launch per block (that kernel adds the
    bias of a one-group launch in another order than a grouped launch's), and the results are the same either way."""
    from bmc_hip import ops
    dev = _gpu()
    monkeypatch.setattr(ops, "WINO_MIN_TILES", 1)
    monkeypatch.setattr(ops, "WINO_MIN_TILES4", 1)
    monkeypatch.setattr(ops, "WINO4_MIN_TILES", 1)
    monkeypatch.setattr(ops, "WINO4", route == 4)
    monkeypatch.setattr(ops, "PAIR_RES", True)
    monkeypatch.setattr(ops, "PAIR_RES_MIN_TILES", 1)
    monkeypatch.setattr(ops, "PAIR_RES_DGRAD", True)
    ops._DENSE.clear()
    B2, Hn, Wn = 4, 36, 52
    blks = _blocks(dev, bias == "zero")
    rules = (blks[0].conv1.bias, blks[1].conv1.bias)
    assert ops.wino_ok(B2, Hn, Wn, CN, 9, fwd=True, stride=CN, rule=rules[0]) == route
    assert ops._pair_route(B2, Hn, Wn, CN, 9, rules, fwd=True) == (0 if (route == 2 and bias == "dense") else route)
    assert ops._pair_route(B2, Hn, Wn, CN, 9) == route
    g = torch.Generator(device=dev).manual_seed(5)
    xb = torch.randn(B2, Hn, Wn, CN, generator=g, device=dev)      # (allocated first)
    xa = torch.randn(B2, Hn, Wn, CN, generator=g, device=dev)
    gy = torch.randn(2 * B2, Hn, Wn, CN, generator=g, device=dev)
    launches = []
    real = ops.conv_raw
    monkeypatch.setattr(ops, "conv_raw", lambda srcs, *a, **k: (launches.append(a[6]), real(srcs, *a, **k))[1])
    ref = _run_node(False, blks, xa, xb, gy, grad)
    n_ref = len(launches)
    got = _run_node(True, blks, xa, xb, gy, grad)
    n_got = len(launches) - n_ref
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
    assert float(ref["y"].abs().max()) > 0.5 and (not grad or float(ref["0.conv1.weight"].abs().max()) > 0)
    # launches through conv_raw: 4 forward + 4 data-gradient ones for the two nodes; the pair shares 2 + 1 of them
    shares = not (route == 2 and bias == "dense")
    assert n_ref == (8 if grad else 4)
    assert n_got == ((5 if shares else 7) if grad else (2 if shares else 4))
