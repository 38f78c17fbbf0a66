"""tests/pgemm_ref.py, the float64 restatement of bmc_pgemm, tied to F.conv2d's autograd and torch.bmm -- and the bars of
tests/test_gpu_pgemm_kernels.py shown to discriminate: every planted defect of pgemm_ref.DEFECTS (a pixel dropped or counted twice, a
tap one column off, a column block read 4 channels off, an image from the wrong group) breaks the integer equality, the fp32
first-order bound and the bf16x6 rel-L2 bar on a 1x1 and on a 3x3 case.  Also: the integer cases are exact in fp32 and bf16, and
the case table reaches every kernel instantiation and every branch the GPU file names.  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import pgemm_ref as R

F64 = torch.float64
BAR_X6 = 3e-6           # the GPU file's bar for bf16x6 (tests/test_gpu_bf16_kernels.py)


def _conv_grads(a_imgs, x_imgs, k):
    """F.conv2d autograd: dW [M][N][k][k], db [M] for dY = a_imgs [b][H][W][M], input x_imgs [b][H][W][N], float64."""
    M, N = a_imgs.shape[-1], x_imgs.shape[-1]
    w = torch.zeros(M, N, k, k, dtype=F64, requires_grad=True)
    b = torch.zeros(M, dtype=F64, requires_grad=True)
    F.conv2d(x_imgs.permute(0, 3, 1, 2), w, b, padding=k // 2).backward(a_imgs.permute(0, 3, 1, 2))
    return w.grad, b.grad


def _close(got, want):
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


# (taps, B, bpg, H, W, M, source windows [(Ct, c0, nch)], source shift, source mod, A as a table, sources as tables)
CONV_CASES = [
    (9, 2, 2, 5, 7, 8, [(12, 4, 8)], 0, None, False, False),
    (1, 2, 2, 5, 7, 8, [(12, 4, 8)], 0, None, False, False),
    (9, 4, 2, 6, 19, 12, [(8, 0, 8), (16, 4, 4), (4, 0, 4)], 0, None, False, False),        # groups, several sources
    (1, 4, 2, 9, 9, 12, [(8, 0, 8), (16, 4, 4), (4, 0, 4)], 0, None, False, False),
    (9, 4, 1, 4, 4, 4, [(8, 4, 4)], 1, 4, False, False),                                     # rotated over the batch
    (1, 4, 2, 3, 17, 4, [(8, 4, 4), (4, 0, 4)], 2, 2, False, False),                         # shifted and wrapped: mod < B
    (9, 3, 3, 1, 1, 4, [(4, 0, 4)], 0, None, True, True),                                    # one-pixel images, table operands
    (1, 4, 2, 2, 33, 8, [(8, 0, 4), (8, 4, 4)], 0, None, True, False),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "taps%d-B%d-bpg%d-%dx%d-shift%d" % (c[0], c[1], c[2], c[3], c[4], c[7]))
def test_reference_equals_conv2d_autograd(case):
    taps, B, bpg, H, W, M, wins, shift, mod, tab_a, tab_x = case
    g = torch.Generator().manual_seed(11 * taps + B + H)
    At = torch.randn(B, H, W, M + 4, dtype=F64, generator=g)
    Bx = mod if mod is not None else B
    Xt = [torch.randn(Bx, H, W, ct, dtype=F64, generator=g) for ct, _, _ in wins]

    def src_image(i, b):
        return Xt[i][(b + shift) % mod if mod is not None else b + shift]

    a = R.Operand(images=[At[b] for b in range(B)], c0=4, nch=M) if tab_a else R.Operand(At, 4, M)
    srcs = [R.Operand(images=[src_image(i, b) for b in range(B)], c0=c0, nch=n) if tab_x else R.Operand(Xt[i], c0, n, shift, mod)
            for i, (_, c0, n) in enumerate(wins)]
    r = R.pgemm(a, srcs, B, H, W, taps, bpg)
    k = 3 if taps == 9 else 1
    G, N = B // bpg, sum(n for _, _, n in wins)
    assert r.C.shape == (G, taps, M, N) and r.db.shape == (G, M)
    for gi in range(G):
        imgs = range(gi * bpg, (gi + 1) * bpg)
        a_imgs = torch.stack([At[b][..., 4:4 + M] for b in imgs])
        x_imgs = torch.stack([torch.cat([src_image(i, b)[..., c0:c0 + n] for i, (_, c0, n) in enumerate(wins)], -1) for b in imgs])
        dw, db = _conv_grads(a_imgs, x_imgs, k)
        _close(r.C[gi], dw.permute(2, 3, 0, 1).reshape(taps, M, N))
        _close(r.db[gi], db)
        dw_abs, db_abs = _conv_grads(a_imgs.abs(), x_imgs.abs(), k)
        _close(r.absC[gi], dw_abs.permute(2, 3, 0, 1).reshape(taps, M, N))
        _close(r.absdb[gi], db_abs)
        dw_one, _ = _conv_grads(torch.ones_like(a_imgs), torch.ones_like(x_imgs), k)          # the number of products
        assert torch.equal(r.count[gi], dw_one.permute(2, 3, 0, 1).reshape(taps, M, N))


def test_reference_equals_bmm_in_gram_form():
    B, H, W, Cn = 3, 6, 11, 20
    g = torch.Generator().manual_seed(5)
    center, v = torch.randn(B, H, W, Cn, dtype=F64, generator=g), torch.randn(B, H, W, Cn, dtype=F64, generator=g)
    r = R.pgemm(R.Operand(center), [R.Operand(v)], B, H, W, 1, 1)
    want = torch.bmm(center.reshape(B, H * W, Cn).transpose(1, 2), v.reshape(B, H * W, Cn))   # center [B][C][HW] . v^T
    _close(r.C[:, 0], want)
    assert torch.equal(r.count, torch.full_like(r.count, H * W))


def test_shifted_is_zero_padded():
    X = torch.arange(1.0, 13.0, dtype=F64).reshape(1, 3, 4, 1)
    assert torch.equal(R.shifted(X, 0, 0), X)
    s = R.shifted(X, 1, -1)[0, :, :, 0]
    assert torch.equal(s, torch.tensor([[0.0, 5, 6, 7], [0, 9, 10, 11], [0, 0, 0, 0]], dtype=F64))
    assert not R.shifted(X[:, :1, :1], 1, 0).any() and not R.shifted(X, 0, 4).any()


# ------------------------------------------------------------------ the GPU file's cases
@pytest.mark.parametrize("shape", sorted(R.SHAPES))
def test_integer_cases_are_exact_in_fp32_and_bf16(shape):
    s = R.SHAPES[shape]
    a, xs = R.operands(shape, "int")
    for t in [a] + xs:
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 8
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    r = R.reference(shape, "int")
    assert float(r.absC.max()) < 2 ** 24 and float(r.absdb.max()) < 2 ** 24
    assert torch.equal(r.C, r.C.round()) and torch.equal(r.db, r.db.round())
    assert s.bpg * s.H * s.W <= 2048                    # what the fp32 bound's discrimination rests on
    assert s.M % 4 == 0 and all(n % 4 == 0 for n in s.widths) and len(s.widths) <= R.MAX_SRC


def _violates_fp32_bound(got, ref):
    return bool(((got.C - ref.C).abs() > ref.count * R.U32 * ref.absC).any())


def _rel_l2(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("defect", R.DEFECTS)
@pytest.mark.parametrize("shape", ["e", "m"])           # a 1x1 and a 3x3 case, two groups each
def test_bars_discriminate(shape, defect):
    s = R.SHAPES[shape]
    for data in ("int", "randn"):
        a, xs = R.operands(shape, data)
        bad = R.pgemm(R.Operand(a), [R.Operand(x) for x in xs], s.B, s.H, s.W, s.taps, s.bpg, defect=defect)
        ref = R.reference(shape, data)
        if data == "int":
            assert not torch.equal(bad.C, ref.C)
        else:
            assert _violates_fp32_bound(bad, ref)
            assert _rel_l2(bad.C, ref.C) > BAR_X6
    ok = R.pgemm(R.Operand(a), [R.Operand(x) for x in xs], s.B, s.H, s.W, s.taps, s.bpg)     # and the bars admit the reference
    assert torch.equal(ok.C, ref.C) and not _violates_fp32_bound(ok, ref)


def test_fp32_bound_sees_one_typical_product():
    """A single dropped or doubled product of typical size (|a x| = E|a| E|x| = 2 / pi for randn) lies above the fp32 bound of every
    randn case: at most 2048 pixels per group."""
    for c in R.CASES:
        if c.data == "randn" and c.math == 0:
            ref = R.reference(c.shape, "randn")
            assert float((ref.count * R.U32 * ref.absC).max()) < 2.0 / 3.141592653589793, c


def _branches(c):
    """Branches of pgemm_dma_kernel a case reaches, restated from its source (fp32 cases)."""
    s = R.SHAPES[c.shape]
    N, tpi = sum(s.widths), R.tiles_per_image(s)
    ntiles, xch = s.bpg * tpi, 64 if s.taps == 9 else 128
    out = set()
    if c.nsplit > ntiles:
        out.add("empty_split")
    if ntiles >= 3 * c.nsplit:
        out.add("buffers_refilled")             # a split with three tiles or more: the double buffer / register ring turns over
    if c.nsplit >= tpi and ntiles > c.nsplit:
        out.add("walk_steps_over_images")
    if R.pad32(s.M) < 128:
        out.add("idle_row_waves")
    if R.wave_map(s.taps, s.M, N) == 4 and R.pad32(N) == 32 and c.tap_groups != 3:
        out.add("ks4_idle_column_waves")
    if s.bias and R.pad32(s.M) > 128 and s.M < R.pad32(s.M):
        out.add("bias_two_row_blocks_padded")
    if s.shift or c.tab:
        out.add("shift_mod" if s.shift else "table_" + c.tab)
    if s.taps == 9:
        interior = any(4 * ty >= 1 and 16 * tx >= 1 and 4 * ty + 5 <= s.H and 16 * tx + 17 <= s.W
                       for ty in range((s.H + 3) // 4) for tx in range((s.W + 15) // 16))
    else:
        interior = s.H * s.W >= 64
    starts, n0 = [0], 0
    for w in s.widths:
        starts.append(starts[-1] + w)
    while n0 < N:
        si = max(i for i in range(len(s.widths)) if starts[i] <= n0)
        if interior and s.M >= 128 and n0 + xch <= starts[si + 1]:
            out.add("uniform_fill")
            if si > 0 and n0 > starts[si]:
                out.add("uniform_fill_inside_a_later_source")
        n0 += xch
    return out


def test_case_table_reaches_every_kernel_and_branch():
    reached = {R.case_kernel(c) for c in R.CASES}
    assert len(R.DMA_KERNELS) == 10 and len(set(R.ALL_KERNELS)) == len(R.ALL_KERNELS) == 18
    assert reached == set(R.ALL_KERNELS), sorted(set(R.ALL_KERNELS) ^ reached)
    for data in ("int", "randn"):               # every fp32 kernel sees both kinds of operands
        assert {R.case_kernel(c) for c in R.CASES if c.math == 0 and c.data == data} == set(R.DMA_KERNELS)
    assert {R.case_kernel(c) for c in R.CASES if c.math == 3 and c.data == "randn"} == {"bf9x3", "bf9x3<tab>", "bf<1,3>", "bf<1,3,tab>"}
    for taps in (1, 9):
        got = set().union(*[_branches(c) for c in R.CASES if c.math == 0 and R.SHAPES[c.shape].taps == taps])
        want = {"empty_split", "walk_steps_over_images", "idle_row_waves", "uniform_fill", "table_all", "buffers_refilled"}
        assert want <= got, (taps, want - got)
        for math in (1, 3):                     # the bf16 kernels: splits without tiles, and tile loads that run ahead of a re-used slot
            ks = [c for c in R.CASES if c.math == math and R.SHAPES[c.shape].taps == taps]
            assert {"empty_split", "buffers_refilled"} <= set().union(*[_branches(c) for c in ks]), (taps, math)
            assert any("buffers_refilled" in _branches(c) and "uniform_fill" in _branches(c) for c in ks), (taps, math)
    all_b = set().union(*[_branches(c) for c in R.CASES if c.math == 0])
    assert {"ks4_idle_column_waves", "bias_two_row_blocks_padded", "shift_mod", "table_a", "uniform_fill_inside_a_later_source"} <= all_b
    assert len({R.case_id(c) for c in R.CASES}) == len(R.CASES)


def test_kernel_names():
    assert R.kernel_name(0, 9, 1, True, 128, 16) == "dma<9,9,tab,ks2>"
    assert R.kernel_name(3, 9, 0, True, 128, 64) == "bf9x3<tab>"
    assert R.kernel_name(0, 9, 0, False, 128, 64) == "dma<9,9>" and R.kernel_name(0, 9, 3, False, 32, 32) == "dma<9,3>"
    assert R.kernel_name(0, 9, 1, False, 32, 32) == "dma<9,9,ks4>" and R.kernel_name(0, 9, 1, False, 33, 32) == "dma<9,9,ks2>"
    assert R.kernel_name(0, 1, 1, False, 32, 32) == "dma<1,1>" and R.kernel_name(1, 9, 3, False, 32, 32) == "bf<9,1>"
    assert R.kernel_name(3, 1, 1, True, 32, 32) == "bf<1,3,tab>" and R.kernel_name(1, 1, 1, False, 32, 32) == "bf<1,1>"


def test_wave_map_agrees_with_the_library():
    """The restated rule against bmc_pgemm_wave_map, where libbmc_hip.so loads on this machine (the GPU file repeats it)."""
    for M, N, want in ((32, 32, 4), (16, 256, 4), (33, 32, 2), (128, 16, 2), (48, 33, 1), (128, 64, 1)):
        assert R.wave_map(9, M, N) == want and R.wave_map(1, M, N) == 1
    try:
        from bmc_hip import lib
    except (ImportError, OSError):
        return
    for taps in (1, 9):
        for M in (4, 16, 32, 36, 48, 64, 128, 160):
            for N in (4, 16, 32, 36, 64, 80, 128, 256, 272):
                assert lib.pgemm_wave_map(taps, M, N) == R.wave_map(taps, M, N), (taps, M, N)
