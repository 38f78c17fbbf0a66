"""The 3x3 pixel-reduction GEMM's wave maps with k-step shares (csrc/pgemm.hip, KS = 2 / 4), each alone against float64.

Launches whose shape leaves waves of the 4 row-block x 2 column-block map without rows or columns of their own -- the narrow
"rest" sources of the split weight gradients (N <= 32) and conv_o (M = 32) -- deal those waves a share of each pixel tile's
k-steps instead; the shares meet in LDS in a fixed order.  ops.pgemm_raw + ops.reduce_wgrad are called directly so the shape under
test is certain, `bmc_pgemm_wave_map` says which map the launcher takes, and the all-taps workgroup is forced at these small
frames (the dispatcher would give them one tap row per workgroup, which keeps the 4 x 2 map).

Bar: rel-L2 < 3e-5 against F.conv2d's float64 gradients, what tests/test_gpu_parity.py holds this kernel family to; two runs
bit-identical."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture()
def all_taps(monkeypatch):
    from bmc_hip import ops
    monkeypatch.setattr(ops, "TAP_SPLIT_TILES", 0)
    monkeypatch.setattr(ops, "MATH", 0)
    return ops


# (name, M, physical source widths, reference channel of every physical column (-1 = padding), expected KS)
SHAPES = {
    "m128_n16": (128, [16], [list(range(16))], 2),
    "m128_n16x2_pad": (128, [16, 16], [list(range(16)), list(range(16, 24)) + [-1] * 8], 2),
    "m32_n128x2": (32, [128, 128], [list(range(128)), list(range(128, 256))], 4),
}
# 9 x 21: boundary tiles and zero-sourced pixels, one tile per split; 4 x 16: one tile per image; the last two: more tiles than
# splits (256 / 64 of them), so tiles are double-buffered and the first splits receive one tile more than the rest
CASES = [(s, 2, 9, 21, b) for s in SHAPES for b in (False, True)] + [(s, 2, 4, 16, True) for s in SHAPES] + \
        [("m128_n16", 2, 36, 240, True), ("m32_n128x2", 2, 20, 100, True)]


@pytest.mark.parametrize("shape,B,H,W,bias", CASES)
def test_wave_map_wgrad_vs_float64(all_taps, shape, B, H, W, bias):
    ops = all_taps
    from bmc_hip import lib
    dev = _gpu()
    M, widths, cols, ks = SHAPES[shape]
    spec = ops.ConvSpec(cols)
    assert lib.pgemm_wave_map(9, M, spec.kpad) == ks
    assert lib.pgemm_wave_map(9, 128, 64) == 1 and lib.pgemm_wave_map(1, 32, 32) == 1
    g = torch.Generator().manual_seed(7)
    dy = torch.randn(B, H, W, M, generator=g)
    xs = [torch.randn(B, H, W, n, generator=g) for n in widths]
    # float64 reference: the sources' real channels, in the weight tensor's column order
    real = torch.cat([x[..., [i for i, c in enumerate(cs) if c >= 0]] for x, cs in zip(xs, cols)], 3)
    x64 = real.permute(0, 3, 1, 2).double()
    w64 = torch.zeros(M, spec.cin, 3, 3, dtype=torch.float64, requires_grad=True)
    b64 = torch.zeros(M, dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, w64, b64, padding=1).backward(dy.permute(0, 3, 1, 2).double())

    dy_g, xs_g = dy.to(dev), [x.to(dev) for x in xs]
    tiles = B * ((H + 3) // 4) * ((W + 15) // 16)

    def run():
        a = ops._src(dy_g, 0, M, 0, None, 0, B)
        r = ops.pgemm_raw(a, [ops._src(x, 0, n, 0, None, 0, B) for x, n in zip(xs_g, widths)], B, H, W, 9, B, M, spec.kpad, dev,
                          want_bias=bias)
        if (H, W) == (36, 240) or (H, W) == (20, 100):
            assert r[1] < tiles and tiles % r[1] != 0       # some splits hold one tile more than others
        dw, db = ops.reduce_wgrad(r[0], r[1], 1, 9, M, spec, dev, r[3] if bias else None, None, None, (M, spec.cin, 3, 3))
        torch.cuda.synchronize()
        return dw, db

    dw, db = run()
    dw2, db2 = run()
    e_w = rel_l2(dw, w64.grad)
    print("%s %dx%dx%d: dW rel-L2 %.2e" % (shape, B, H, W, e_w))
    assert e_w < 3e-5
    assert torch.equal(dw, dw2)
    if bias:
        e_b = rel_l2(db, b64.grad)
        print("%s %dx%dx%d: db rel-L2 %.2e" % (shape, B, H, W, e_b))
        assert e_b < 3e-5
        assert torch.equal(db, db2)
