"""Plain restatements of the weight-path entry points of include/bmc_hip.h: the layout kernels every convolution weight passes
on its way into an MFMA kernel (bmc_pack_weight, bmc_pack_weight_t, bmc_pack_weight_wino, bmc_pack_weight_wino4,
bmc_split_weight) and the reductions every weight gradient passes on its way out (bmc_pgemm_reduce_weight[_groups],
bmc_pgemm_reduce_plain, bmc_wgrad_wino_reduce).  One function per entry point, written from the header's description of the
layout: a dense, zero-padded operator is built first and then reshaped / permuted into the streaming order; torch on the CPU, sums
and transforms in float64 (int64 for integer inputs), no tiling, no fixed summation order.  The two plain packs only move data and
keep the dtype of their input.  tests/test_weight_path_ref_cpu.py ties every function here to F.conv2d / autograd in float64;
tests/test_gpu_weight_path_kernels.py checks the kernels against these functions."""
import numpy as np
import torch

F64 = torch.float64
CK = 16
SWZ = (0, 2, 3, 1)          # quad swizzle of a 16-float row of the F(2x2) pack, indexed by (row >> 2) & 3


def lavin_G(m):
    """G of F(m x m, 3 x 3) as published (Lavin & Gray 2015): the matrix of tests/wino_numerics.py::lavin, [m + 2][3] float64."""
    import wino_numerics
    return torch.tensor(wino_numerics.lavin(m)[1], dtype=F64)


def _wide(t):
    t = t.detach().cpu()
    return t.to(F64) if t.is_floating_point() else t.to(torch.int64)


def _kmap(kmap, n, Cin):
    """The first n entries of the map packed channel -> reference input channel.  None: the header's implicit map, k -> k for
    k < Cin and -1 (zero) for k >= Cin, in every pack, forward and transposed (the kernels guard both)."""
    if kmap is None:
        return torch.tensor([k if k < Cin else -1 for k in range(n)], dtype=torch.int64)
    km = torch.as_tensor(kmap).detach().cpu().to(torch.int64).reshape(-1)
    assert km.numel() >= n and int(km.max()) < Cin
    return km[:n]


# ------------------------------------------------------------------ the two plain packs
def pack_weight(w, kmap, Kpad, Coutpad):
    """w [G][Cout][Cin][taps] -> [G][Kpad/16][taps][Coutpad][16]: packed input channel k holds reference channel kmap[k], zero
    where kmap[k] < 0, for output rows >= Cout and (kmap None) for k >= Cin."""
    w = w.detach().cpu()
    G, Cout, Cin, taps = w.shape
    km = _kmap(kmap, Kpad, Cin)
    real = (km >= 0).nonzero().reshape(-1)
    dense = torch.zeros(G, Kpad, taps, Coutpad, dtype=w.dtype)              # [g][k][tap][co]
    dense[:, real, :, :Cout] = w[:, :, km[real], :].permute(0, 2, 3, 1)
    return dense.reshape(G, Kpad // CK, CK, taps, Coutpad).permute(0, 1, 3, 4, 2).contiguous()


def pack_weight_t(w, kmap, k0, nk, nkpad, Coutpad16):
    """The data-gradient operator of packed source channels [k0, k0 + nk): [G][Coutpad16/16][taps][nkpad][16], output rows
    n = k - k0 (zero for n >= nk, for holes of the map and, under the implicit map, for k0 + n >= Cin), reduction over the Cout
    output channels (zero for co >= Cout), taps mirrored."""
    w = w.detach().cpu()
    G, Cout, Cin, taps = w.shape
    km = _kmap(kmap, k0 + nk, Cin)[k0:]
    real = (km >= 0).nonzero().reshape(-1)
    dense = torch.zeros(G, Coutpad16, taps, nkpad, dtype=w.dtype)           # [g][co][tap][n]
    dense[:, :Cout, :, real] = w[:, :, km[real], :].flip(-1).permute(0, 1, 3, 2)
    return dense.reshape(G, Coutpad16 // CK, CK, taps, nkpad).permute(0, 1, 3, 4, 2).contiguous()


# ------------------------------------------------------------------ the two Winograd packs
def _wino_operator(w, kmap, Kpad, rows, transposed, k0, nk):
    """The zero-padded 3x3 filters behind a Winograd pack, float64 [G][rows][Kpad][3][3]: forward rows = output channels, K = packed
    input channels through kmap; transposed rows = packed source channels k0 + n (n < nk), K = output channels, taps mirrored.
    Holes of the map, and channels >= Cin under the implicit map (kmap None), are zero filters in both forms."""
    w = w.detach().cpu().to(F64)
    G, Cout, Cin = w.shape[:3]
    w = w.reshape(G, Cout, Cin, 3, 3)
    g = torch.zeros(G, rows, Kpad, 3, 3, dtype=F64)
    if not transposed:
        km = _kmap(kmap, Kpad, Cin)
        real = (km >= 0).nonzero().reshape(-1)
        g[:, :Cout, real] = w[:, :, km[real]]
    else:
        km = _kmap(kmap, k0 + nk, Cin)[k0:]
        real = (km >= 0).nonzero().reshape(-1)
        g[:, real, :Cout] = w[:, :, km[real]].flip(-1, -2).transpose(1, 2)
    return g


def _wino_U(g, m, absolute=False):
    """U = G g G^T per filter: [G][rows][K][3][3] -> [G][K][n][n][rows], n = m + 2 (absolute: the sum of the terms' magnitudes)."""
    Gm = lavin_G(m)
    if absolute:
        g, Gm = g.abs(), Gm.abs()
    return torch.einsum("xi,grkij,nj->gkxnr", Gm, g, Gm)


def pack_wino(w, kmap, Kpad, Coutpad, transposed=0, k0=0, nk=0):
    """U = G g G^T of F(2x2, 3x3) in float64 -> [G][Kpad/16][4 (xi)][4 (nu)][rows = Coutpad][16]; the four 4-float quads of a row
    are stored XOR-swizzled: quad q of row r sits at quad q ^ SWZ[(r >> 2) & 3]."""
    G = w.shape[0]
    U = _wino_U(_wino_operator(w, kmap, Kpad, Coutpad, transposed, k0, nk), 2)              # [G][K][4][4][rows]
    U = U.reshape(G, Kpad // CK, CK, 4, 4, Coutpad).permute(0, 1, 3, 4, 5, 2)               # [G][chunk][xi][nu][row][16]
    src = torch.tensor([[((j >> 2) ^ SWZ[(r >> 2) & 3]) * 4 + (j & 3) for j in range(CK)] for r in range(Coutpad)])
    return torch.gather(U, 5, src.expand(U.shape)).contiguous()


def pack_wino4(w, kmap, Kpad, Coutpad, transposed=0, k0=0, nk=0, absolute=False):
    """U = G g G^T of F(4x4, 3x3) in float64 -> [G][Coutpad/128][Kpad/16][8 (wave)][36 (position)][64 (lane)][4]: lane l of wave v
    holds row 128 ntile + 16 v + (l & 15), channels 16 chunk + 4 (l >> 4) + 0 .. 3.  absolute: the same layout holding the sum of
    the magnitudes of the 9 terms of every element (for an evaluation-order bound)."""
    G = w.shape[0]
    U = _wino_U(_wino_operator(w, kmap, Kpad, Coutpad, transposed, k0, nk), 4, absolute)    # [G][K][6][6][rows]
    U = U.reshape(G, Kpad // CK, 4, 4, 36, Coutpad // 128, 8, 16)          # [g][chunk][quad][c][pos][ntile][wave][r16]
    return U.permute(0, 5, 1, 6, 4, 2, 7, 3).reshape(G, Coutpad // 128, Kpad // CK, 8, 36, 64, 4).contiguous()


# ------------------------------------------------------------------ fp32 -> bf16 planes
def _swap_halves(rows16, Coutpad):
    """[..][Coutpad][16]: the two 8-value halves of a row change places when (row & 16) -- its own inverse."""
    odd = ((torch.arange(Coutpad) & 16) != 0).view(-1, 1)
    return torch.where(odd, torch.cat([rows16[..., 8:], rows16[..., :8]], -1), rows16)


def split_weight(packed, Coutpad, planes):
    """packed fp32 [nsteps][Coutpad][16] -> int16 bit patterns [nsteps][planes][Coutpad][16]: plane p = the running residual rounded
    to bf16 (nearest even, torch's conversion), the residual then reduced by exactly that value (taken in float64; it is a multiple
    of the input's last bit and below 2^-8 of it, so always a float32 again -- subnormals included, which the CPU keeps)."""
    r = packed.detach().cpu().to(torch.float32).reshape(-1, Coutpad, CK).clone()
    out = []
    for _ in range(planes):
        b = r.to(torch.bfloat16)
        out.append(_swap_halves(b.view(torch.int16), Coutpad))
        r64 = r.to(F64) - b.to(F64)
        r = r64.to(torch.float32)
        assert torch.equal(r.to(F64), r64), "the residual is not exact"
    return torch.stack(out, 1).contiguous()


def split_planes_values(bits, Coutpad, planes):
    """The bf16 planes of split_weight / bmc_split_weight as float64 values [nsteps][planes][Coutpad][16], halves put back."""
    b = torch.as_tensor(bits).detach().cpu().contiguous().view(torch.int16).reshape(-1, planes, Coutpad, CK)
    return _swap_halves(b, Coutpad).contiguous().view(torch.bfloat16).to(F64)


# ------------------------------------------------------------------ slab reductions
def _pad32(v):
    return (v + 31) // 32 * 32


def reduce_weight(slabs, nsplit, G, taps, M, N, kmap, Cin, prior=None, accumulate=0, bias_slabs=None, prior_b=None):
    """slabs [nsplit][G][taps][Mpad][Npad] (Mpad / Npad = M / N rounded up to 32) -> dW [G][M][Cin][taps]: column kmap[n] (=|+=)
    the sum over the splits of slab column n; columns the map does not name keep `prior`.  kmap None: column n -> n, which the
    header allows only for N <= Cin (the entry points refuse the rest).  bias_slabs [nsplit][G][4][Mpad] ->
    db [G][M] (=|+=) the sum over splits and the 4 parts.  -> (dW, db or None), float64 (int64 for integer inputs)."""
    s = _wide(slabs).reshape(nsplit, G, taps, _pad32(M), _pad32(N))[:, :, :, :M, :N].sum(0)         # [G][taps][M][N]
    assert kmap is not None or N <= Cin
    km = _kmap(kmap, N, Cin)
    real = (km >= 0).nonzero().reshape(-1)
    dw = _wide(prior).reshape(G, M, Cin, taps).clone() if prior is not None else torch.zeros(G, M, Cin, taps, dtype=s.dtype)
    new = s[:, :, :, real].permute(0, 2, 3, 1).to(dw.dtype)                                         # [G][M][named][taps]
    dw[:, :, km[real], :] = dw[:, :, km[real], :] + new if accumulate else new
    db = None
    if bias_slabs is not None:
        db = _wide(bias_slabs).reshape(nsplit, G, 4, _pad32(M))[:, :, :, :M].sum((0, 2))
        if accumulate:
            pb = _wide(prior_b).reshape(G, M)
            db = db.to(pb.dtype) + pb
    return dw, db


def reduce_plain(slabs, nsplit, G, M, N, scale):
    """slabs [nsplit][G][Mpad][Npad] -> out [G][M][N] = (sum over the splits) * scale, scale as the float32 the entry point takes."""
    s = _wide(slabs).reshape(nsplit, G, _pad32(M), _pad32(N))[:, :, :M, :N].sum(0)
    return s if scale == 1 else s * float(np.float32(scale))


def wino_wgrad_reduce(part, nsplit, prior, ldw, k0, accumulate=0, bias_part=None, prior_b=None):
    """part [nsplit][16 (xi, nu)][128 co][128 ci] -> dW [128][ldw][3][3]: columns [k0, k0 + 128) (=|+=) G'^T (sum of dU) G', every
    other column keeps `prior`.  G' = the G of F(2x2, 3x3) whose LAST ROW enters with -1: the main kernel leaves out the sign of the
    rows of A that are a lone -1, so the partial sums of positions xi = 3 or nu = 3 arrive with the opposite sign.
    bias_part [nsplit][128] -> db [128] (=|+=) its sum.  -> (dW, db or None) in float64."""
    dU = part.detach().cpu().to(F64).reshape(nsplit, 4, 4, 128, 128).sum(0)
    Gp = lavin_G(2) * torch.tensor([1.0, 1.0, 1.0, -1.0], dtype=F64).view(4, 1)
    new = torch.einsum("xi,xnkc,nj->kcij", Gp, dU, Gp)
    dw = prior.detach().cpu().to(F64).reshape(128, ldw, 3, 3).clone() if prior is not None else torch.zeros(128, ldw, 3, 3, dtype=F64)
    dw[:, k0:k0 + 128] = dw[:, k0:k0 + 128] + new if accumulate else new
    db = None
    if bias_part is not None:
        db = bias_part.detach().cpu().to(F64).reshape(nsplit, 128).sum(0)
        if accumulate:
            db = db + prior_b.detach().cpu().to(F64).reshape(128)
    return dw, db


# ------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
def example_kmaps(Kpad, seed):
    """name -> (kmap or None, Cin): dense, with holes (a run of -1 in the middle and at the end of a 16-chunk), a strict subset of
    Cin out of order, and the implicit map with Cin < Kpad."""
    g = torch.Generator().manual_seed(seed)
    holed, c = [], 0
    for k in range(Kpad):
        if 5 <= k % 16 <= 8 or k % 16 >= 14:
            holed.append(-1)
        else:
            holed.append(c)
            c += 1
    subset = torch.randperm(Kpad + 9, generator=g)[:Kpad].tolist()
    return {"dense": (list(range(Kpad)), Kpad), "holed": (holed, c), "subset": (subset, Kpad + 9), "null": (None, Kpad - 5)}


def wide_range_values(n, seed, lo=-100, hi=101):
    g = torch.Generator().manual_seed(seed)
    mant = 1 + torch.randint(0, 2 ** 23, (n,), generator=g).double() / 2 ** 23
    e = torch.randint(lo, hi, (n,), generator=g)
    sgn = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    x = torch.ldexp(sgn * mant, e).float()
    assert bool(((x.abs() >= 2.0 ** lo) & (x.abs() < 2.0 ** hi)).all())
    return x
