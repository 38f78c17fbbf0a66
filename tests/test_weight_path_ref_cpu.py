"""tests/weight_path_ref.py is itself checked, without a GPU: every restatement is tied to F.conv2d / autograd in float64, so that
the GPU tests (tests/test_gpu_weight_path_kernels.py) cannot merely agree with a wrong layout.  The layouts are undone here by
explicit index loops written from include/bmc_hip.h, not with the reference's own reshapes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import weight_path_ref as R
import wino_numerics as WN

F64 = torch.float64


def _named(kmap, Kpad, Cin):
    return [(k, (kmap[k] if kmap is not None else (k if k < Cin else -1))) for k in range(Kpad)]


def _packed_input(x_ref, kmap, Kpad):
    """The packed source tensor of a launch: channel k carries reference channel kmap[k]; holes carry garbage that only zero
    weights may meet."""
    B, Cin, H, W = x_ref.shape
    xp = torch.randn(B, Kpad, H, W, dtype=F64, generator=torch.Generator().manual_seed(5)) * 100
    for k, ci in _named(kmap, Kpad, Cin):
        if ci >= 0:
            xp[:, k] = x_ref[:, ci]
    return xp


@pytest.mark.parametrize("taps", [1, 9])
@pytest.mark.parametrize("kind", ["dense", "holed", "subset", "null"])
def test_pack_weight_contracted_with_im2col_is_conv2d(kind, taps):
    G, Cout, Coutpad, Kpad, B, H, W = 2, 20, 32, 32, 2, 5, 6
    kmap, Cin = R.example_kmaps(Kpad, 1)[kind]
    torch.manual_seed(3)
    w = torch.randn(G, Cout, Cin, taps, dtype=F64)
    P = R.pack_weight(w, kmap, Kpad, Coutpad)
    assert P.shape == (G, Kpad // 16, taps, Coutpad, 16) and P.dtype == w.dtype
    assert bool((P[:, :, :, Cout:] == 0).all())
    x_ref = torch.randn(B, Cin, H, W, dtype=F64)
    xp = _packed_input(x_ref, kmap, Kpad)
    k = 3 if taps == 9 else 1
    cols = F.unfold(xp, k, padding=k // 2).reshape(B, Kpad // 16, 16, taps, H * W)          # [b][chunk][kk][tap][pixel]
    named = sorted(ci for _, ci in _named(kmap, Kpad, Cin) if ci >= 0)
    for g in range(G):
        got = torch.einsum("ctok,bcktp->bop", P[g], cols)[:, :Cout].reshape(B, Cout, H, W)
        want = F.conv2d(x_ref[:, named], w[g][:, named].reshape(Cout, len(named), k, k), padding=k // 2)
        assert float((got - want).abs().max()) < 1e-9


@pytest.mark.parametrize("taps", [1, 9])
@pytest.mark.parametrize("kind,k0,nk,nkpad", [("dense", 0, 16, 32), ("holed", 16, 48, 128), ("subset", 16, 16, 32), ("null", 16, 48, 128)])
def test_pack_weight_t_contracted_with_im2col_is_the_data_gradient(kind, k0, nk, nkpad, taps):
    G, Cout, Kpad, B, H, W = 2, 20, 64, 2, 5, 6
    c16 = 32
    kmap, Cin = R.example_kmaps(Kpad, 2)[kind]                              # null: Cin = 59 < k0 + nk = 64, rows 43 .. 47 are zero
    torch.manual_seed(4)
    w = torch.randn(G, Cout, Cin, taps, dtype=F64)
    T = R.pack_weight_t(w, kmap, k0, nk, nkpad, c16)
    assert T.shape == (G, c16 // 16, taps, nkpad, 16)
    k = 3 if taps == 9 else 1
    dy = torch.randn(B, Cout, H, W, dtype=F64)
    dyp = torch.cat([dy, torch.randn(B, c16 - Cout, H, W, dtype=F64) * 100], 1)             # pad channels: garbage x zero weights
    cols = F.unfold(dyp, k, padding=k // 2).reshape(B, c16 // 16, 16, taps, H * W)
    for g in range(G):
        x = torch.randn(B, Cin, H, W, dtype=F64, requires_grad=True)
        (dx,) = torch.autograd.grad(F.conv2d(x, w[g].reshape(Cout, Cin, k, k), padding=k // 2), x, dy)
        got = torch.einsum("ctnk,bcktp->bnp", T[g], cols).reshape(B, nkpad, H, W)
        for n in range(nkpad):
            ci = _named(kmap, Kpad, Cin)[k0 + n][1] if n < nk else -1
            want = dx[:, ci] if ci >= 0 else torch.zeros(B, H, W, dtype=F64)
            assert float((got[:, n] - want).abs().max()) < 1e-9, (n, ci)


def _unpack_wino2(P, G, Kpad, rows):
    """[G][Kpad/16][4][4][rows][16] with the {0, 2, 3, 1} quad swizzle -> U[g][k][xi][nu][row], by the header's words."""
    P = P.reshape(G, Kpad // 16, 4, 4, rows, 16)
    U = torch.zeros(G, Kpad, 4, 4, rows, dtype=F64)
    table = (0, 2, 3, 1)
    for row in range(rows):
        s = table[(row >> 2) & 3]
        for kk in range(16):
            at = ((kk >> 2) ^ s) * 4 + (kk & 3)
            for c in range(Kpad // 16):
                U[:, c * 16 + kk, :, :, row] = P[:, c, :, :, row, at]
    return U


def _unpack_wino4(P, G, Kpad, rows):
    """[G][rows/128][Kpad/16][8][36][64][4] -> U[g][k][xi][nu][row]: lane l of wave v = row 128 ntile + 16 v + (l & 15), channels
    16 chunk + 4 (l >> 4) + 0 .. 3."""
    P = P.reshape(G, rows // 128, Kpad // 16, 8, 36, 64, 4)
    U = torch.zeros(G, Kpad, 6, 6, rows, dtype=F64)
    for nt in range(rows // 128):
        for c in range(Kpad // 16):
            for v in range(8):
                for lane in range(64):
                    row = 128 * nt + 16 * v + (lane & 15)
                    for j in range(4):
                        U[:, 16 * c + 4 * (lane >> 4) + j, :, :, row] = P[:, nt, c, v, :, lane, j].reshape(G, 6, 6)
    return U


WINO_CASES = [  # Cout, Kpad, rows (Coutpad), transposed, k0, nk, kmap kind, length of the map
    (20, 32, 128, 0, 0, 0, "holed", 32),
    (20, 32, 128, 0, 0, 0, "subset", 32),
    (20, 16, 128, 0, 0, 0, "null", 16),
    (20, 32, 128, 1, 16, 40, "holed", 64),
    (20, 32, 128, 1, 0, 16, "subset", 64),
    (20, 32, 128, 1, 16, 48, "null", 64),                                   # Cin = 59 < k0 + nk = 64: rows 43 .. 47 are zero
]


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("Cout,Kpad,rows,transposed,k0,nk,kind,klen", WINO_CASES)
def test_winograd_packs_give_the_direct_correlation_on_one_tile(Cout, Kpad, rows, transposed, k0, nk, kind, klen, m):
    G = 2
    kmap, Cin = R.example_kmaps(klen, 6)[kind]
    torch.manual_seed(7 + m)
    w = torch.randn(G, Cout, Cin, 9, dtype=F64)
    AT, _, BT = (torch.tensor(a, dtype=F64) for a in WN.lavin(m))
    n = m + 2
    if m == 2:
        U = _unpack_wino2(R.pack_wino(w, kmap, Kpad, rows, transposed, k0, nk), G, Kpad, rows)
    else:
        U = _unpack_wino4(R.pack_wino4(w, kmap, Kpad, rows, transposed, k0, nk), G, Kpad, rows)
    d = torch.randn(Kpad, n, n, dtype=F64)                                                  # one input tile per K channel
    V = torch.einsum("xi,kij,nj->kxn", BT, d, BT)
    w5 = w.reshape(G, Cout, Cin, 3, 3)
    names = _named(kmap, klen, Cin)
    for g in range(G):
        Y = torch.einsum("ix,xnr,jn->rij", AT, (U[g] * V.unsqueeze(-1)).sum(0), AT)         # [row][m][m]
        want = torch.zeros(rows, m, m, dtype=F64)
        if not transposed:                                                  # rows = output channels, K = packed input channels
            ks = [k for k, ci in names[:Kpad] if ci >= 0]
            cis = [names[k][1] for k in ks]
            want[:Cout] = F.conv2d(d[ks].unsqueeze(0), w5[g][:, cis])[0]
        else:                                                               # rows = source channels k0 + row, K = output channels
            ns = [r for r in range(nk) if names[k0 + r][1] >= 0]
            cis = [names[k0 + r][1] for r in ns]
            want[ns] = F.conv2d(d[:Cout].unsqueeze(0), w5[g][:, cis].flip(-1, -2).transpose(0, 1))[0]
        assert float((Y - want).abs().max()) < 1e-9, g
        assert float(want.abs().max()) > 0.1


def test_wino4_absolute_terms_bound_the_value():
    torch.manual_seed(9)
    w = torch.randn(1, 20, 16, 9, dtype=F64)
    U, A = R.pack_wino4(w, None, 16, 128), R.pack_wino4(w, None, 16, 128, absolute=True)
    assert U.shape == A.shape and bool((A >= U.abs() - 1e-15).all()) and float(A.max()) > 0


def test_f2x2_transform_of_multiples_of_four_is_exact_in_fp32():
    """Weights 4 x integers in [-16, 16]: every intermediate of G g G^T, in the order a float32 evaluation takes, is an integer
    below 2^24 -- the float32 evaluation equals the float64 one bit for bit, whatever the order."""
    g = torch.Generator().manual_seed(11)
    w = (4 * torch.randint(-16, 17, (1, 48, 16, 9), generator=g)).float()
    U64 = R.pack_wino(w, None, 16, 128)
    assert torch.equal(U64, U64.round()) and float(U64.abs().max()) <= 64 * 2.25
    w3 = w.reshape(48, 16, 3, 3)
    half = torch.tensor(0.5)
    rows = [w3[:, :, 0], half * ((w3[:, :, 0] + w3[:, :, 1]) + w3[:, :, 2]), half * ((w3[:, :, 0] - w3[:, :, 1]) + w3[:, :, 2]), w3[:, :, 2]]
    gg = torch.stack(rows, 2)                                                               # [co][ci][xi][3], float32
    cols = [gg[..., 0], half * ((gg[..., 0] + gg[..., 1]) + gg[..., 2]), half * ((gg[..., 0] - gg[..., 1]) + gg[..., 2]), gg[..., 2]]
    U32 = torch.stack(cols, 3)                                                              # [co][ci][xi][nu]
    assert U32.dtype == torch.float32
    want = torch.einsum("xi,okij,nj->okxn", R.lavin_G(2), w3.double(), R.lavin_G(2))
    assert torch.equal(U32.double(), want)
    assert torch.equal(_unpack_wino2(U64, 1, 16, 128)[0, :, :, :, :48].permute(3, 0, 1, 2), want)


# ------------------------------------------------------------------ reductions
def _pad32(v):
    return (v + 31) // 32 * 32


@pytest.mark.parametrize("taps", [1, 9])
@pytest.mark.parametrize("kind", ["dense", "holed", "subset", "null"])
@pytest.mark.parametrize("nsplit", [1, 5])
def test_reduce_weight_of_pixel_subset_gemms_is_autograds_weight_gradient(nsplit, kind, taps):
    G, M, N, B, H, W = 2, 20, 16, 2, 4, 5                                   # B = images per group
    kmap, Cin = R.example_kmaps(N, 8)[kind]
    if kmap is None:
        Cin = N + 3
    names = _named(kmap, N, Cin)
    k = 3 if taps == 9 else 1
    torch.manual_seed(13)
    x_ref = torch.randn(G, B, Cin, H, W, dtype=F64)
    dy = torch.randn(G, B, M, H, W, dtype=F64)
    npix = B * H * W
    owner = torch.randint(0, nsplit, (npix,))                               # an arbitrary split of the pixels
    Mp, Np = _pad32(M), _pad32(N)
    slabs = torch.full((nsplit, G, taps, Mp, Np), float("nan"), dtype=F64)
    bias = torch.full((nsplit, G, 4, Mp), float("nan"), dtype=F64)
    prior = torch.randn(G, M, Cin, taps, dtype=F64)
    prior_b = torch.randn(G, M, dtype=F64)
    want_w, want_b = [], []
    for g in range(G):
        xp = _packed_input(x_ref[g], kmap, N)
        cols = F.unfold(xp, k, padding=k // 2).reshape(B, N, taps, H * W).permute(0, 3, 2, 1).reshape(npix, taps, N)
        a = dy[g].permute(0, 2, 3, 1).reshape(npix, M)
        for s in range(nsplit):
            sel = owner == s
            slabs[s, g, :, :M, :N] = torch.einsum("pm,ptn->tmn", a[sel], cols[sel])
            for part in range(4):
                bias[s, g, part, :M] = a[sel][part::4].sum(0)
        wp = torch.zeros(M, Cin, k, k, dtype=F64, requires_grad=True)
        bp = torch.zeros(M, dtype=F64, requires_grad=True)
        (F.conv2d(x_ref[g], wp, bp, padding=k // 2) * dy[g]).sum().backward()
        want_w.append(wp.grad.reshape(M, Cin, taps))
        want_b.append(bp.grad)
    want_w, want_b = torch.stack(want_w), torch.stack(want_b)
    named = torch.zeros(Cin, dtype=torch.bool)
    named[[ci for _, ci in names if ci >= 0]] = True
    for acc in (0, 1):
        dw, db = R.reduce_weight(slabs, nsplit, G, taps, M, N, kmap, Cin, prior, acc, bias, prior_b)
        assert dw.shape == (G, M, Cin, taps) and db.shape == (G, M)
        assert float((dw[:, :, named] - (want_w + acc * prior)[:, :, named]).abs().max()) < 1e-9
        assert torch.equal(dw[:, :, ~named], prior[:, :, ~named])           # columns the map does not name keep their value
        assert float((db - (want_b + acc * prior_b)).abs().max()) < 1e-9
    dw, db = R.reduce_weight(slabs, nsplit, G, taps, M, N, kmap, Cin)       # no prior, no bias
    assert db is None and float((dw[:, :, named] - want_w[:, :, named]).abs().max()) < 1e-9


def test_reduce_weight_sums_integers_in_int64():
    g = torch.Generator().manual_seed(17)
    v = torch.randint(-64, 65, (7, 1, 1, 32, 32), generator=g)
    dw, _ = R.reduce_weight(v, 7, 1, 1, 20, 16, None, 16)
    assert dw.dtype == torch.int64 and torch.equal(dw[0, :, :, 0], v[:, 0, 0, :20, :16].sum(0))


@pytest.mark.parametrize("scale", [1.0, 128 ** -0.5])
def test_reduce_plain_is_the_scaled_gram_matrix(scale):
    G, M, N, nsplit, npix = 2, 20, 33, 5, 40
    torch.manual_seed(19)
    a, b = torch.randn(G, npix, M, dtype=F64), torch.randn(G, npix, N, dtype=F64)
    owner = torch.randint(0, nsplit, (npix,))
    slabs = torch.full((nsplit, G, _pad32(M), _pad32(N)), float("nan"), dtype=F64)
    for s in range(nsplit):
        slabs[s, :, :M, :N] = torch.einsum("gpm,gpn->gmn", a[:, owner == s], b[:, owner == s])
    got = R.reduce_plain(slabs, nsplit, G, M, N, scale)
    want = torch.einsum("gpm,gpn->gmn", a, b) * float(np.float32(scale))
    assert got.shape == (G, M, N) and float((got - want).abs().max()) < 1e-9


@pytest.mark.parametrize("nsplit", [1, 3])
def test_wino_wgrad_reduce_of_float64_partials_is_autograds_weight_gradient(nsplit):
    """Partial sums as the main kernel leaves them -- dU over subsets of the tiles, the positions xi = 3 / nu = 3 with the sign of
    A's lone -1 left out -- reduce to autograd's weight gradient: this pins the -1 convention of the reduction."""
    B, H, W, C = 2, 5, 7, 128
    torch.manual_seed(23)
    x = torch.randn(B, C, H, W, dtype=F64) * (torch.rand(B, C, H, W) < 0.5)
    g = torch.randn(B, C, H, W, dtype=F64)
    AT, _, BT = (torch.tensor(a, dtype=F64) for a in WN.lavin(2))
    t, th, tw = WN.tiles_of(x, 2)
    V = torch.einsum("ai,bcyxij,dj->adbyxc", BT, t, BT).reshape(4, 4, -1, C)                 # [xi][nu][tile][ci]
    gt, _, _ = WN.out_tiles_of(g, 2)
    sign = torch.tensor([1.0, 1.0, 1.0, -1.0], dtype=F64)
    Aleft = AT.t() * sign.view(4, 1)                                                         # A with its lone -1 row left positive
    dM = torch.einsum("ai,bkyxij,dj->adbyxk", Aleft, gt, Aleft).reshape(4, 4, -1, C)         # [xi][nu][tile][co]
    ntile = V.shape[2]
    owner = torch.randint(0, nsplit, (ntile,))
    part = torch.stack([torch.einsum("xntk,xntc->xnkc", dM[:, :, owner == s], V[:, :, owner == s]) for s in range(nsplit)])
    bias_part = torch.stack([gt.permute(0, 2, 3, 4, 5, 1).reshape(ntile, 4, C)[owner == s].sum((0, 1)) for s in range(nsplit)])
    wp = torch.zeros(C, C, 3, 3, dtype=F64, requires_grad=True)
    bp = torch.zeros(C, dtype=F64, requires_grad=True)
    (F.conv2d(x, wp, bp, padding=1) * g).sum().backward()
    ldw, k0 = 160, 16
    prior = torch.randn(C, ldw, 3, 3, dtype=F64)
    prior_b = torch.randn(C, dtype=F64)
    for acc in (0, 1):
        dw, db = R.wino_wgrad_reduce(part, nsplit, prior, ldw, k0, acc, bias_part, prior_b)
        assert float((dw[:, k0:k0 + C] - (wp.grad + acc * prior[:, k0:k0 + C])).abs().max()) < 1e-9
        assert torch.equal(dw[:, :k0], prior[:, :k0]) and torch.equal(dw[:, k0 + C:], prior[:, k0 + C:])
        assert float((db - (bp.grad + acc * prior_b)).abs().max()) < 1e-9
    plain = torch.einsum("xntk,xntc->xnkc", dM * (sign.view(4, 1, 1, 1) * sign.view(1, 4, 1, 1)), V)
    G2 = R.lavin_G(2)
    assert float((torch.einsum("xi,xnkc,nj->kcij", G2, plain, G2) - wp.grad).abs().max()) < 1e-9     # the unsigned textbook form


# ------------------------------------------------------------------ bf16 planes
def _check_split(x, Coutpad):
    bits3 = R.split_weight(x, Coutpad, 3)                                    # raises if a residual is not a float32
    bits1 = R.split_weight(x, Coutpad, 1)
    assert bits3.dtype == torch.int16 and bits3.shape == (x.numel() // (Coutpad * 16), 3, Coutpad, 16)
    assert torch.equal(bits1[:, 0], bits3[:, 0])
    v = R.split_planes_values(bits3, Coutpad, 3)
    x64 = x.double().reshape(-1, Coutpad, 16)
    assert torch.equal(v.sum(1), x64)                                        # the planes sum to the input exactly ...
    assert torch.equal((x64 - v[:, 0]) - v[:, 1] - v[:, 2], torch.zeros_like(x64))   # ... and the third residual is zero
    assert torch.equal(v[:, 0], x.reshape(-1, Coutpad, 16).to(torch.bfloat16).double())
    return bits3


def test_split_weight_planes_sum_exactly_over_the_exponent_range():
    x = R.wide_range_values(400 * 1024, 29)                                   # 4.1e5 values, 2^-100 <= |x| < 2^101
    _check_split(x, 128)


def test_split_weight_mantissa_sweep_ties_zeros_and_the_half_swap():
    m = torch.arange(0, 2 ** 23, 257, dtype=torch.int32)                     # a sweep of the 23 mantissa bits (and all of the low 16)
    low = torch.arange(0, 2 ** 16, dtype=torch.int32)
    x = torch.cat([(m | 0x3F800000).view(torch.float32), (low | 0x40000000).view(torch.float32),
                   torch.tensor([0.0, -0.0, 1.5, -3.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -10])])
    x = torch.cat([x, torch.zeros(-x.numel() % (32 * 16))])
    bits = _check_split(x, 32)
    flat = R.split_planes_values(bits, 32, 3).reshape(-1, 3, 32 * 16)
    sp = m.numel() + low.numel()
    row, col = sp // 512, sp % 512
    got = flat[row, :, col:col + 7]
    assert got[0].tolist() == [0.0, 0.0, 1.5, -3.0, 1.0, 1 + 2.0 ** -6, 1.0]                 # ties go to the even bf16
    assert got[1].tolist() == [0.0, 0.0, 0.0, 0.0, 2.0 ** -8, -2.0 ** -8, 2.0 ** -10] and bool((got[2] == 0).all())
    assert bool(torch.signbit(got[0, 1])) and not bool(torch.signbit(got[0, 0]))             # -0.0 keeps its sign bit
    # the half swap: rows with bit 4 set store values 8 .. 15 first
    y = torch.arange(2 * 32 * 16, dtype=torch.float32)
    b = R.split_weight(y, 32, 1).view(torch.bfloat16).float().reshape(2, 32, 16)
    for r in range(32):
        want = y.reshape(2, 32, 16)[1, r].to(torch.bfloat16).float()
        want = torch.cat([want[8:], want[:8]]) if r & 16 else want
        assert torch.equal(b[1, r], want)
