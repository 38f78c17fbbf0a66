"""Every weight-path kernel alone: the layout kernels a convolution weight passes on its way into an MFMA kernel (bmc_pack_weight,
bmc_pack_weight_t of csrc/stream_ops.hip; bmc_pack_weight_wino of csrc/wino.hip; bmc_pack_weight_wino4 of csrc/wino4.hip;
bmc_split_weight of csrc/conv_bf.hip) and the reductions a weight gradient passes on its way out (bmc_pgemm_reduce_weight,
_groups, _plain of csrc/pgemm.hip; bmc_wgrad_wino, _multi, _reduce of csrc/wino_wgrad.hip), against their restatements in
tests/weight_path_ref.py -- which tests/test_weight_path_ref_cpu.py ties to F.conv2d / autograd in float64.

Every output buffer is a Guarded buffer whose payload is pre-filled with NaN (its guards keep SENT): a pad element the kernel
does not write, or writes as anything but 0.0, fails the comparison, as it would poison an MFMA kernel that multiplies it by a zero
activation once recycled memory holds a NaN there.  Every input pad the kernel must not use (slab rows >= M, slab columns >= N,
bias-slab rows >= M) is NaN as well.

Bit-exact (torch.equal on the whole buffer): the two plain packs; the F(2x2) pack on weights 4 x integers in [-16, 16] (every
intermediate of G g G^T is then an integer: tests/test_weight_path_ref_cpu.py); the bf16 planes; every reduction on integer-valued
slabs (|v| <= 64, sums below 2^24: any order is exact); the run-to-run identity of every reduction; the grouped reduction against
the ungrouped one; the multi-pair F(2x2) weight gradient against the single-pair entry on the concatenated operands.
Bounds fixed in advance, nothing measured: the F(4x4) pack |got - ref64| <= 2^-24 |ref64| + 2^-49 sum|terms| (one fp32 rounding
plus the double-precision evaluation-order slack); randn slabs |got - ref64| <= (nsplit + 1) 2^-24 sum|terms| (4 nsplit + 1 for
the bias): the order-free first-order bound of a sum.
The F(2x2) weight gradient is held to the 4x rule of tests/test_gpu_streaming_kernels.py: its largest elementwise error against
float64 (test_gpu_r3._wgrad_reference) is at most 4x that of wino_numerics.wino_wgrad -- the same algorithm in fp32 on the CPU --
with a floor of 1 ulp of the largest |reference|; the bias gradient 4x ATen's sum of the same terms.

Launch arithmetic the shapes come from:
  * pack_weight / pack_weight_t: min(ceil(n / 256), MAXBLK = 2048) blocks of 256, grid-stride: G = 1, Kpad = Coutpad = 256,
    taps = 9 is 589 824 elements, above 2048 * 256 = 524 288;
  * the two Winograd packs cap their grid at 65 535 blocks of 256 threads, one thread per (row, K channel): reaching the cap needs
    more than 16.7 M pairs, an output above 1 GB.  NOT TESTED here: their grid-stride loop runs one iteration in every case;
  * reduce_weight4_kernel (N % 4 == 0): P = 1, 2, 4, 8, 16, 32 threads share an output quad's splits at nsplit <= 4, 8, 16, 64,
    128, > 128, each in a 4 P-unrolled loop plus tail; reduce_weight_kernel (else), reduce_plain_kernel: 8 parts, stride 8;
    bias_block_sum: 64 parts over 4 nsplit partials, its 8 x 64-unrolled body runs from nsplit >= 113;
  * wino_wgrad_kernel: a stage = 4 rows x 16 columns of pixels, stages = B ceil(ceil(H/2)/2) ceil(ceil(W/2)/8), split s takes
    stages [stages s / nsplit, stages (s + 1) / nsplit); the workgroup -> (split, xi) map changes at nsplit % 8 == 0;
    wino_wgrad_reduce_kernel: 8 parts over the splits (weights), 2 (bias).

bmc_split_weight below 2^-100: a residual of such an input can be a float32 subnormal.  Those inputs are run and what is seen is
printed (SPLIT_SMALL), not asserted.  Seen on an MI355X: nothing is flushed -- all three planes of all 2048 normal inputs in
[2^-126, 2^-100) and of all 512 subnormal inputs equal the CPU reference bit for bit.  The planes of such inputs no longer sum to
the input (882 of the 2048 do, none of the subnormal ones), on the GPU as on the CPU: a residual below 2^-126 is a bf16
subnormal, which keeps bits down to 2^-133 only.

F(4x4) pack, seen on an MI355X (WINO4_PACK): 0.03 - 0.21 % of the elements of a case (its pads counted) are one fp32 ulp away from
the rounded float64 reference (near-ties, decided by the evaluation order in double); none is outside the bound.

Measured on an MI355X: every `RATIO` line that vs_aten prints (pytest -s), 52 comparisons in all; per group the number of
comparisons, the largest ratio and the case that has it.  The bound is 4.

RATIO_TABLE_BEGIN
group                      cases  max ratio  at
wgrad_wino dW                 13       1.82  B=3 13x37 nsplit=1
wgrad_wino db                 13       1.87  B=1 4x16 nsplit=1
wgrad_wino_reduce dW          12       0.63  k0=160 acc=1 bias=0
wgrad_wino_reduce db           6       0.58  k0=0 acc=0 bias=1
wgrad_wino_multi dW            4       0.58  nseg=8 nsplit=11
wgrad_wino_multi db            4       1.37  nseg=1 nsplit=6

cases with ratio >= 2: none
RATIO_TABLE_END

Findings.  No kernel failed a bar on the cases above as first written, but writing them turned up two defects of the NULL kmap:
  * transposed packs (pack_weight_t_kernel, and the transposed branches of pack_wino_kernel / pack_wino4_kernel) took
    ci = k0 + n without the `< Cin` guard of the forward packs: with k0 + nk > Cin they read the next output channel's weights,
    and past the end of w for the last row.  Found by reading; the unguarded kernels were NOT run on such a case (an
    out-of-bounds read), so there are no figures from before the fix.  All three now read `k0 + n < Cin ? k0 + n : -1`, the
    header states the implicit map once for every pack, and the NULL cases here have Cin < k0 + nk (zero rows past Cin);
  * bmc_pgemm_reduce_weight[_groups] with a NULL kmap write column n of a Cin-column row: N > Cin was neither documented nor
    checked.  The header now requires N <= Cin and both entry points refuse the rest (test_reduce_weight*_refuses).
And one of the header: the F(2x2) pack's swizzle sentence named (row >> 2) & 3 where the kernels use {0, 2, 3, 1}[(row >> 2) & 3].
"""
import ctypes as C

import pytest
import torch

import weight_path_ref as R
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_streaming_kernels import GUARD, SENT, Guarded, call, refused, ulp32, vs_aten  # noqa: F401

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN = float("nan")


# ------------------------------------------------------------------ helpers
def nan_out(n, dev, init=None):
    """A Guarded output buffer whose payload is NaN (or `init`): every element has to be written."""
    g = Guarded(n, dev)
    if init is None:
        g.t.fill_(NAN)
    else:
        g.t.copy_(init.reshape(-1))
    return g


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _dev_kmap(kmap, dev):
    return None if kmap is None else torch.tensor(kmap, dtype=torch.int32, device=dev)


def _p(t):
    return None if t is None else (t.ptr() if isinstance(t, Guarded) else t.data_ptr())


def _pad32(v):
    return (v + 31) // 32 * 32


def _named_columns(kmap, N, Cin):
    named = torch.zeros(Cin, dtype=torch.bool)
    named[[c for c in (kmap if kmap is not None else range(N))[:N] if c >= 0]] = True
    return named


# ================================================================== bmc_pack_weight, bmc_pack_weight_t
PACK_ROWS = [(16, 32), (48, 128), (128, 128)]                               # narrow tile, pad rows, no pad


def _weights(G, Cout, Cin, taps, dev, seed):
    torch.manual_seed(seed)
    w = torch.randn(G, Cout, Cin, taps, device=dev)
    w.view(-1)[:2] = torch.tensor([-0.0, 1e-42], device=dev)                # a copy keeps the sign of zero and a subnormal
    return w


def _pack_direct(w, kmap, Kpad, Coutpad, dev):
    G, Cout, Cin, taps = w.shape
    km = _dev_kmap(kmap, dev)
    out = nan_out(G * Kpad * taps * Coutpad, dev)
    call("_pack_w", "bmc_pack_weight", w.data_ptr(), _p(km), G, Cout, Cin, taps, Kpad, Coutpad, out.ptr())
    return out.cpu()


def _pack_t_direct(w, kmap, k0, nk, nkpad, c16, dev):
    G, Cout, Cin, taps = w.shape
    km = _dev_kmap(kmap, dev)
    out = nan_out(G * c16 * taps * nkpad, dev)
    call("_pack_wt", "bmc_pack_weight_t", w.data_ptr(), _p(km), G, Cout, Cin, taps, k0, nk, nkpad, c16, out.ptr())
    return out.cpu()


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("taps", [1, 9])
@pytest.mark.parametrize("Cout,Coutpad", PACK_ROWS)
def test_pack_weight_bit_exact(Cout, Coutpad, taps, G):
    dev = _gpu()
    Kpad = 48
    for kind, (kmap, Cin) in R.example_kmaps(Kpad, Cout + taps).items():
        w = _weights(G, Cout, Cin, taps, dev, Cout * 10 + taps + G)
        got = _pack_direct(w, kmap, Kpad, Coutpad, dev)
        want = R.pack_weight(w.cpu(), kmap, Kpad, Coutpad).reshape(-1)
        assert same_bits(got, want), kind


def test_pack_weight_above_one_grid_pass():
    dev = _gpu()
    w = _weights(1, 250, 250, 9, dev, 5)                                    # kmap NULL, Cin < Kpad, 6 pad rows
    got = _pack_direct(w, None, 256, 256, dev)
    assert got.numel() == 589824 > 2048 * 256
    assert same_bits(got, R.pack_weight(w.cpu(), None, 256, 256).reshape(-1))


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("taps", [1, 9])
@pytest.mark.parametrize("Cout", [16, 20, 48, 128])                         # 20: Coutpad16 = 32 > Cout
def test_pack_weight_t_bit_exact(Cout, taps, G):
    dev = _gpu()
    c16 = (Cout + 15) // 16 * 16
    for kind, (kmap, Cin) in R.example_kmaps(64, Cout + taps + 1).items():      # NULL: Cin = 59, the windows ending at 64 pass it
        w =_weights(G, Cout, Cin, taps, dev, Cout * 10 + taps + G + 1)
        for k0 in (0, 16):
            for nk, nkpad in ((16, 32), (48, 128)):
                got = _pack_t_direct(w, kmap, k0, nk, nkpad, c16, dev)
                want = R.pack_weight_t(w.cpu(), kmap, k0, nk, nkpad, c16).reshape(-1)
                assert same_bits(got, want), (kind, k0, nk)


def test_pack_weight_t_above_one_grid_pass():
    dev = _gpu()
    w = _weights(1, 250, 256, 9, dev, 6)
    got = _pack_t_direct(w, None, 0, 250, 256, 256, dev)
    assert got.numel() == 589824
    assert same_bits(got, R.pack_weight_t(w.cpu(), None, 0, 250, 256, 256).reshape(-1))


def test_pack_wrappers_launch_the_same_kernels():
    dev = _gpu()
    from bmc_hip import ops
    ops.set_math("fp32")
    kmap, c = R.example_kmaps(48, 3)["holed"]
    spec = ops.ConvSpec([kmap[:32], kmap[32:]], cin=c + 3)                  # holes, and three columns no source names
    w = _weights(2, 48, c + 3, 9, dev, 7)
    got = ops._packed_weight(w, spec, None).cpu()
    assert same_bits(got, _pack_direct(w, kmap, 48, 128, dev))
    got = ops._packed_weight_t(w, spec, 1, None).cpu()
    assert same_bits(got, _pack_t_direct(w, kmap, 32, 16, 32, 48, dev))


def test_pack_weight_refuses():
    dev = _gpu()
    w = torch.ones(16 * 16 * 9, device=dev)
    out = Guarded(4096, dev)
    refused("_pack_w", "bmc_pack_weight", w.data_ptr(), None, 1, 16, 16, 1, 40, 32, out.ptr(), match="Kpad % 16 / Coutpad % 32")
    refused("_pack_w", "bmc_pack_weight", w.data_ptr(), None, 1, 16, 16, 1, 16, 48, out.ptr(), match="Kpad % 16 / Coutpad % 32")
    assert out.untouched()


def test_pack_weight_t_refuses():
    dev = _gpu()
    w = torch.ones(16 * 16 * 9, device=dev)
    out = Guarded(4096, dev)
    refused("_pack_wt", "bmc_pack_weight_t", w.data_ptr(), None, 1, 16, 16, 1, 0, 16, 32, 24, out.ptr(), match="Coutpad16 % 16")
    refused("_pack_wt", "bmc_pack_weight_t", w.data_ptr(), None, 1, 16, 16, 1, 0, 16, 48, 16, out.ptr(), match="nkpad % 32")
    assert out.untouched()


# ================================================================== bmc_pack_weight_wino, bmc_pack_weight_wino4
WINO_CASES = [  # G, Cout, Kpad, rows (Coutpad), transposed, k0, nk, kmap kind, length of the map
    (1, 48, 16, 128, 0, 0, 0, "dense", 16),
    (2, 128, 48, 128, 0, 0, 0, "holed", 48),
    (1, 128, 128, 256, 0, 0, 0, "subset", 128),
    (2, 48, 48, 256, 0, 0, 0, "null", 48),                                  # Cin = 43 < Kpad
    (1, 48, 48, 128, 1, 0, 48, "dense", 64),
    (2, 40, 48, 128, 1, 16, 48, "holed", 64),                               # Kpad > Cout, nk < rows
    (1, 128, 128, 256, 1, 16, 144, "subset", 160),
    (1, 16, 16, 128, 1, 0, 16, "null", 16),                                 # Cin = 11 < k0 + nk: rows 11 .. 15 are zero
    (2, 40, 48, 128, 1, 16, 48, "null", 64),                                # Cin = 59 < k0 + nk = 64, k0 > 0
]


def _wino_case(case, dev, integer):
    G, Cout, Kpad, rows, transposed, k0, nk, kind, klen = case
    kmap, Cin = R.example_kmaps(klen, Cout + Kpad)[kind]
    torch.manual_seed(Cout + Kpad + rows + transposed)
    if integer:
        w = (4 * torch.randint(-16, 17, (G, Cout, Cin, 9))).float().to(dev)
    else:
        w = torch.randn(G, Cout, Cin, 9, device=dev)
    return w, kmap, _dev_kmap(kmap, dev), (G, Cout, Cin, Kpad, rows, transposed, k0, nk)


@pytest.mark.parametrize("case", WINO_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_pack_weight_wino_bit_exact_on_multiples_of_four(case):
    dev = _gpu()
    w, kmap, km, (G, Cout, Cin, Kpad, rows, transposed, k0, nk) = _wino_case(case, dev, True)
    out = nan_out(G * Kpad * 16 * rows, dev)
    call("_pack_wino", "bmc_pack_weight_wino", w.data_ptr(), _p(km), G, Cout, Cin, Kpad, rows, transposed, k0, nk, out.ptr())
    want = R.pack_wino(w.cpu(), kmap, Kpad, rows, transposed, k0, nk).reshape(-1)
    got = out.cpu()
    assert torch.equal(got.double(), want)
    assert float(want.abs().max()) >= 16                                    # the case is not empty


@pytest.mark.parametrize("case", WINO_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_pack_weight_wino4_one_rounding_of_float64(case):
    dev = _gpu()
    w, kmap, km, (G, Cout, Cin, Kpad, rows, transposed, k0, nk) = _wino_case(case, dev, False)
    out = nan_out(G * Kpad * 36 * rows, dev)
    call("_pack_wino4", "bmc_pack_weight_wino4", w.data_ptr(), _p(km), G, Cout, Cin, Kpad, rows, transposed, k0, nk, out.ptr())
    ref = R.pack_wino4(w.cpu(), kmap, Kpad, rows, transposed, k0, nk).reshape(-1)
    terms = R.pack_wino4(w.cpu(), kmap, Kpad, rows, transposed, k0, nk, absolute=True).reshape(-1)
    got = out.cpu().double()
    err, bound = (got - ref).abs(), 2.0 ** -24 * ref.abs() + 2.0 ** -49 * terms
    off = int((got != ref.float().double()).sum())
    print("WINO4_PACK %s: %d of %d elements differ from the rounded float64 reference, worst err/bound %.3f"
          % (case, off, got.numel(), float((err / bound.clamp_min(1e-300)).nan_to_num(1e9).max())))
    assert bool((err <= bound).all())                                       # pads: bound 0 -> exactly 0.0 (a NaN fails)
    assert bool((got[terms == 0] == 0).all()) and int((terms == 0).sum()) > 0


@pytest.mark.parametrize("fn,name", [("_pack_wino", "bmc_pack_weight_wino"), ("_pack_wino4", "bmc_pack_weight_wino4")])
def test_pack_weight_wino_refuses(fn, name):
    dev = _gpu()
    w = torch.ones(48 * 48 * 9, device=dev)
    out = Guarded(4096, dev)
    p = w.data_ptr()
    refused(fn, name, p, None, 1, 48, 48, 48, 64, 0, 0, 0, out.ptr(), match="multiple of 128")
    refused(fn, name, p, None, 1, 48, 48, 40, 128, 0, 0, 0, out.ptr(), match="multiple of 16")
    for k0, nk, Kpad in ((0, 0, 48), (0, 129, 48), (-1, 16, 48), (0, 16, 32)):   # empty, wider than the rows, negative, Kpad < Cout
        refused(fn, name, p, None, 1, 48, 48, Kpad, 128, 1, k0, nk, out.ptr(), match="bad transposed window")
    assert out.untouched()


# ================================================================== bmc_split_weight
def _split_input(n, seed):
    x = R.wide_range_values(n, seed, -100, 100)                              # 2^-100 <= |x| < 2^100
    special = torch.tensor([0.0, -0.0, 1.5, -3.0, 2.0 ** -60 * 1.25,        # zeros, exact bf16 values,
                            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2.0 ** 90 * (1 + 3 * 2.0 ** -8),   # ties of both parities,
                            1 + 2.0 ** -10, -(2.0 ** 40) * (1 + 2.0 ** -9 + 2.0 ** -15)])                          # second residual zero
    x[:special.numel()] = special
    x[-special.numel():] = special.flip(0)
    return x


def _split_direct(x, nsteps, Coutpad, planes, dev):
    out = nan_out(nsteps * planes * Coutpad * 8, dev)
    call("_split_w", "bmc_split_weight", x.data_ptr(), out.ptr(), nsteps, Coutpad, planes)
    return out.cpu().view(torch.int16).reshape(nsteps, planes, Coutpad, 16)


@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("nsteps", [1, 9, 145])
@pytest.mark.parametrize("Coutpad", [32, 128])
def test_split_weight_bit_exact(Coutpad, nsteps, planes):
    dev = _gpu()
    from bmc_hip import ops
    xc = _split_input(nsteps * Coutpad * 16, Coutpad + nsteps)
    x = xc.to(dev)
    got = _split_direct(x, nsteps, Coutpad, planes, dev)
    assert torch.equal(got, R.split_weight(xc, Coutpad, planes))
    if planes == 3:                                                          # on the kernel's own result: an exact split
        assert torch.equal(R.split_planes_values(got, Coutpad, 3).sum(1), xc.double().reshape(nsteps, Coutpad, 16))
    ops.set_math(planes)
    w = ops._split_planes(x, Coutpad).cpu().view(torch.int16).reshape(nsteps, planes, Coutpad, 16)
    assert torch.equal(w, got)


def test_split_weight_below_two_to_minus_100_is_reported():
    dev = _gpu()
    g = torch.Generator().manual_seed(3)
    small = R.wide_range_values(32 * 16 * 4, 41, -126, -100)
    sub = torch.randint(1, 2 ** 23, (32 * 16,), generator=g, dtype=torch.int32).view(torch.float32)
    xc = torch.cat([small, sub])
    got = _split_direct(xc.to(dev), 5, 32, 3, dev)
    want = R.split_weight(xc, 32, 3)
    v = R.split_planes_values(got, 32, 3)
    x64 = xc.double().reshape(5, 32, 16)
    for name, sl in (("normal inputs in [2^-126, 2^-100)", slice(0, 4)), ("subnormal inputs", slice(4, 5))):
        n = x64[sl].numel()
        print("SPLIT_SMALL %s: %d values; planes equal to the CPU reference %d %d %d; planes summing to the input exactly %d"
              % (name, n, *[int((got[sl, p] == want[sl, p]).sum()) for p in range(3)], int((v[sl].sum(1) == x64[sl]).sum())))


def test_split_weight_refuses():
    dev = _gpu()
    x = torch.ones(48 * 16, device=dev)
    out = Guarded(4096, dev)
    refused("_split_w", "bmc_split_weight", x.data_ptr(), out.ptr(), 1, 32, 2, match="planes must be 1 or 3")
    refused("_split_w", "bmc_split_weight", x.data_ptr(), out.ptr(), 1, 48, 3, match="bad arguments")
    assert out.untouched()


# ================================================================== slab reductions
NSPLITS = [1, 4, 5, 8, 9, 16, 17, 64, 65, 112, 113, 128, 129, 256]          # both sides of every reduce_parts regime; bias body
RW_SHAPES = [(1, 1, 32, 32), (2, 9, 16, 48), (1, 9, 48, 16), (3, 1, 20, 36)]
# (kmap, accumulate, bias): every kmap with both accumulate values and with and without bias
RW_COMBOS = [("dense", 0, 1), ("holed", 1, 1), ("subset", 0, 0), ("null", 1, 0),
             ("dense", 1, 0), ("holed", 0, 0), ("subset", 1, 1), ("null", 0, 1)]


def _padded(vals, fill):
    """vals [..., M, N] -> [..., Mpad, Npad] with `fill` in the pad rows and columns."""
    M, N = vals.shape[-2:]
    out = torch.full(vals.shape[:-2] + (_pad32(M), _pad32(N)), fill, dtype=vals.dtype)
    out[..., :M, :N] = vals
    return out


def _slab_data(integer, nsplit, G, taps, M, N, seed):
    """-> (slabs, bias slabs) as the float32 images the kernel reads, NaN in every pad row and column, and as the reference's
    inputs (int64 with a garbage pad for the integer kind, float64 with NaN pads else).  Bias slabs: [nsplit][G][4][Mpad]."""
    g = torch.Generator().manual_seed(seed)
    bias_image = lambda b, fill: _padded(b.unsqueeze(-2), fill)[..., 0, :].contiguous()     # pad the M axis only
    if integer:
        v = torch.randint(-64, 65, (nsplit, G, taps, M, N), generator=g)
        b = torch.randint(-64, 65, (nsplit, G, 4, M), generator=g)
        ref = _padded(v, 12345), bias_image(b, 12345)
    else:
        v = torch.randn(nsplit, G, taps, M, N, generator=g)
        b = torch.randn(nsplit, G, 4, M, generator=g)
        ref = _padded(v.double(), NAN), bias_image(b.double(), NAN)
    return (_padded(v.float(), NAN), bias_image(b.float(), NAN)), ref


def _prior(integer, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1000, 1001, shape, generator=g).float() if integer else torch.randn(shape, generator=g) * 5


def _within(got, ref, terms, roundings, what):
    err, bound = (got.double() - ref).abs(), roundings * 2.0 ** -24 * terms
    ok = err <= bound
    assert bool(ok.all()), (what, float(err[~ok].max()) if bool((~ok).any()) else NAN)


def _reduce_weight_case(nsplit, G, taps, M, N, combos, seed):
    dev = _gpu()
    for integer in (True, False):
        (s32, b32), (sref, bref) = _slab_data(integer, nsplit, G, taps, M, N, seed + integer)
        sd, bd = s32.to(dev), b32.to(dev)
        sabs, babs = sref.abs(), bref.abs()
        for kind, acc, bias in combos:
            kmap, Cin = R.example_kmaps(N, seed)[kind]
            Cin = N + 3 if kmap is None else Cin                            # a NULL kmap needs N <= Cin (header; refused else): 3 columns unnamed
            km = _dev_kmap(kmap, dev)
            named = _named_columns(kmap, N, Cin)
            init = _prior(integer, (G, M, Cin, taps), seed + 1)
            init_b = _prior(integer, (G, M), seed + 2)
            if not acc:                                                     # what the call must overwrite starts as NaN
                init[:, :, named] = NAN
                init_b[:] = NAN
            what = "nsplit=%d G=%d taps=%d M=%d N=%d %s acc=%d bias=%d int=%d" % (nsplit, G, taps, M, N, kind, acc, bias, integer)
            runs = []
            for _ in range(1 if integer else 2):
                dw, db = nan_out(init.numel(), dev, init), nan_out(init_b.numel(), dev, init_b)
                call("_red_w", "bmc_pgemm_reduce_weight", sd.data_ptr(), nsplit, G, taps, M, N, _p(km), Cin, dw.ptr(), acc,
                     _p(bd) if bias else None, db.ptr() if bias else None)
                runs.append((dw.cpu(init.shape), db.cpu(init_b.shape)))
            gw, gb = runs[0]
            assert all(same_bits(gw, r[0]) and same_bits(gb, r[1]) for r in runs[1:]), what     # run-to-run identical
            assert same_bits(gw[:, :, ~named], init[:, :, ~named]), what    # columns the map does not name: untouched
            if not bias:
                assert same_bits(gb, init_b), what
            rw, rb = R.reduce_weight(sref, nsplit, G, taps, M, N, kmap, Cin, init, acc, bref if bias else None, init_b)
            if integer:
                assert torch.equal(gw[:, :, named].double(), rw[:, :, named].double()), what
                assert not bias or torch.equal(gb.double(), rb.double()), what
            else:
                tw, tb = R.reduce_weight(sabs, nsplit, G, taps, M, N, kmap, Cin, init.abs(), acc, babs if bias else None, init_b.abs())
                _within(gw[:, :, named], rw[:, :, named], tw[:, :, named], nsplit + 1, what)
                if bias:
                    _within(gb, rb, tb, 4 * nsplit + 1, what + " db")


@pytest.mark.parametrize("G,taps,M,N", RW_SHAPES)
@pytest.mark.parametrize("nsplit", NSPLITS)
def test_reduce_weight(nsplit, G, taps, M, N):
    _reduce_weight_case(nsplit, G, taps, M, N, RW_COMBOS, nsplit * 7 + M + N)


@pytest.mark.parametrize("G,taps,M,N", [(1, 9, 20, 18), (2, 1, 16, 33)])    # N % 4 != 0: the scalar kernel
@pytest.mark.parametrize("nsplit", [1, 8, 9, 113])
def test_reduce_weight_scalar_kernel(nsplit, G, taps, M, N):
    _reduce_weight_case(nsplit, G, taps, M, N, RW_COMBOS, nsplit * 5 + M + N)


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("nsplit", NSPLITS)
def test_reduce_weight_groups_equal_the_ungrouped_call(nsplit, G):
    dev = _gpu()
    taps, M, N = 9, 16, 48
    (s32, b32), _ = _slab_data(False, nsplit, G, taps, M, N, nsplit + G)
    sd, bd = s32.to(dev), b32.to(dev)
    for kind, acc, bias in (("holed", 0, 1), ("subset", 1, 1), ("null", 1, 0)):
        kmap, Cin = R.example_kmaps(N, nsplit)[kind]
        Cin = N + 3 if kmap is None else Cin
        km = _dev_kmap(kmap, dev)
        init, init_b = _prior(False, (G, M, Cin, taps), 5), _prior(False, (G, M), 6)
        if not acc:
            init[:, :, _named_columns(kmap, N, Cin)] = NAN
            init_b[:] = NAN
        dw, db = nan_out(init.numel(), dev, init), nan_out(init_b.numel(), dev, init_b)
        call("_red_w", "bmc_pgemm_reduce_weight", sd.data_ptr(), nsplit, G, taps, M, N, _p(km), Cin, dw.ptr(), acc,
             _p(bd) if bias else None, db.ptr() if bias else None)
        dws = [nan_out(init[g].numel(), dev, init[g]) for g in range(G)]    # every destination its own guarded buffer
        dbs = [nan_out(M, dev, init_b[g]) for g in range(G)]
        PA = C.c_void_p * G
        call("_red_wg", "bmc_pgemm_reduce_weight_groups", sd.data_ptr(), nsplit, G, taps, M, N, _p(km), Cin,
             PA(*[d.ptr() for d in dws]), acc, _p(bd) if bias else None, PA(*[d.ptr() for d in dbs]) if bias else None)
        gw, gb = dw.cpu(init.shape), db.cpu(init_b.shape)
        for g in range(G):
            assert same_bits(dws[g].cpu(init[g].shape), gw[g]) and same_bits(dbs[g].cpu(), gb[g]), (kind, acc, bias, g)


@pytest.mark.parametrize("scale", [1.0, 128 ** -0.5])
@pytest.mark.parametrize("nsplit", [1, 7, 8, 9, 64, 200])
@pytest.mark.parametrize("G,M,N", [(1, 16, 16), (2, 48, 33), (4, 128, 128)])
def test_reduce_plain(G, M, N, nsplit, scale):
    dev = _gpu()
    for integer in (True, False):
        (s32, _), (sref, _) = _slab_data(integer, nsplit, G, 1, M, N, nsplit + M + integer)
        sd = s32.to(dev)
        runs = []
        for _ in range(2):
            out = nan_out(G * M * N, dev)
            call("_red_p", "bmc_pgemm_reduce_plain", sd.data_ptr(), nsplit, G, M, N, scale, out.ptr())
            runs.append(out.cpu((G, M, N)))
        assert same_bits(runs[0], runs[1])
        ref = R.reduce_plain(sref, nsplit, G, M, N, scale)
        if integer and scale == 1.0:
            assert torch.equal(runs[0].double(), ref.double())
        else:
            terms = R.reduce_plain(sref.abs(), nsplit, G, M, N, scale)
            _within(runs[0], ref.double(), terms.double(), nsplit + 1, "plain G=%d M=%d N=%d nsplit=%d int=%d" % (G, M, N, nsplit, integer))


def test_reduce_weight_refuses():
    dev = _gpu()
    s = torch.ones(2 * 32 * 32, device=dev)
    b = torch.ones(2 * 4 * 32, device=dev)
    dw, db = Guarded(16 * 16, dev), Guarded(16, dev)
    refused("_red_w", "bmc_pgemm_reduce_weight", s.data_ptr(), 2, 1, 1, 16, 16, None, 16, dw.ptr(), 0, b.data_ptr(), None,
            match="bias_slabs and db go together")
    refused("_red_w", "bmc_pgemm_reduce_weight", s.data_ptr(), 2, 1, 1, 16, 16, None, 16, dw.ptr(), 0, None, db.ptr(),
            match="bias_slabs and db go together")
    refused("_red_w", "bmc_pgemm_reduce_weight", s.data_ptr(), 0, 1, 1, 16, 16, None, 16, dw.ptr(), 0, None, None, match="bad args")
    refused("_red_w", "bmc_pgemm_reduce_weight", s.data_ptr(), 2, 1, 1, 16, 16, None, 16, None, 0, None, None, match="bad args")
    refused("_red_w", "bmc_pgemm_reduce_weight", s.data_ptr(), 2, 1, 1, 16, 16, None, 15, dw.ptr(), 0, None, None,
            match="NULL kmap needs N <= Cin")
    assert dw.untouched() and db.untouched()


def test_reduce_weight_groups_refuses():
    dev = _gpu()
    s = torch.ones(2 * 5 * 32 * 32, device=dev)
    b = torch.ones(2 * 5 * 4 * 32, device=dev)
    dws, dbs = [Guarded(16 * 16, dev) for _ in range(5)], [Guarded(16, dev) for _ in range(5)]
    P5, P2 = C.c_void_p * 5, C.c_void_p * 2
    w5, b5 = P5(*[d.ptr() for d in dws]), P5(*[d.ptr() for d in dbs])
    args = (s.data_ptr(), 2, 5, 1, 16, 16, None, 16, w5, 0, b.data_ptr(), b5)
    refused("_red_wg", "bmc_pgemm_reduce_weight_groups", *args, match="1 <= G <= 4")
    refused("_red_wg", "bmc_pgemm_reduce_weight_groups", s.data_ptr(), 2, 2, 1, 16, 16, None, 16, P2(dws[0].ptr(), None), 0, None, None,
            match="null destination for group 1")
    refused("_red_wg", "bmc_pgemm_reduce_weight_groups", s.data_ptr(), 2, 2, 1, 16, 16, None, 16, w5, 0, b.data_ptr(),
            P2(None, dbs[1].ptr()), match="null destination for group 0")
    refused("_red_wg", "bmc_pgemm_reduce_weight_groups", s.data_ptr(), 2, 2, 1, 16, 16, None, 16, w5, 0, b.data_ptr(), None,
            match="bias_slabs and db go together")
    refused("_red_wg", "bmc_pgemm_reduce_weight_groups", s.data_ptr(), 2, 2, 1, 16, 16, None, 16, w5, 0, None, b5,
            match="bias_slabs and db go together")
    refused("_red_wg", "bmc_pgemm_reduce_weight_groups", s.data_ptr(), 2, 2, 1, 16, 16, None, 15, w5, 0, None, None,
            match="NULL kmap needs N <= Cin")
    assert all(d.untouched() for d in dws + dbs)


def test_reduce_plain_refuses():
    dev = _gpu()
    s = torch.ones(2 * 32 * 32, device=dev)
    out = Guarded(16 * 16, dev)
    refused("_red_p", "bmc_pgemm_reduce_plain", s.data_ptr(), 0, 1, 16, 16, 1.0, out.ptr(), match="bad args")
    refused("_red_p", "bmc_pgemm_reduce_plain", None, 2, 1, 16, 16, 1.0, out.ptr(), match="bad args")
    refused("_red_p", "bmc_pgemm_reduce_plain", s.data_ptr(), 2, 1, 16, 16, 1.0, None, match="bad args")
    assert out.untouched()


# ================================================================== F(2x2) Winograd weight gradient
_SCHEME = []


def _emulation(x, g):
    """wino_numerics.wino_wgrad: the same algorithm in fp32 on the CPU.  x, g NHWC -> dW [co][ci][3][3]."""
    import wino_numerics as WN
    if not _SCHEME:
        _SCHEME.append(WN.Scheme("F(2x2,3x3)", 2, WN.lavin(2)))
    return WN.wino_wgrad(x.cpu().permute(0, 3, 1, 2).contiguous(), g.cpu().permute(0, 3, 1, 2).contiguous(), _SCHEME[0])


def _stages(B, H, W):
    return B * (((H + 1) // 2 + 1) // 2) * (((W + 1) // 2 + 7) // 8)


def _operands(B, H, W, dev, seed):
    torch.manual_seed(seed)
    return torch.randn(B, H, W, 128, device=dev), torch.randn(B, H, W, 128, device=dev)


def _ww_launch(g, x, nsplit, bias, dev):
    from bmc_hip import ops
    B, H, W, _ = x.shape
    a_src, x_src = ops._src(g, 0, 128, 0, None, 0, B), ops._src(x, 0, 128, 0, None, 0, B)
    part = nan_out(nsplit * 16 * 128 * 128, dev)
    bpart = nan_out(nsplit * 128, dev) if bias else None
    call("_ww", "bmc_wgrad_wino", C.byref(a_src), C.byref(x_src), B, H, W, nsplit, part.ptr(), _p(bpart))
    return part, bpart


def _ww_reduce(part, nsplit, dw, ldw, k0, acc, bpart=None, db=None):
    call("_ww_red", "bmc_wgrad_wino_reduce", _p(part), nsplit, dw.ptr(), ldw, k0, int(acc), _p(bpart), _p(db))


WW_CASES = [(1, 1, 1, 1), (1, 4, 16, 1), (2, 5, 17, 1), (2, 5, 17, 8), (3, 7, 33, 5), (3, 7, 33, 18)] + \
           [(3, 13, 37, n) for n in (1, 3, 7, 8, 9, 17, 36)]


@pytest.mark.parametrize("B,H,W,nsplit", WW_CASES)
def test_wgrad_wino_elementwise_vs_float64_and_bit_identical(B, H, W, nsplit):
    dev = _gpu()
    from test_gpu_r3 import _wgrad_reference
    assert 1 <= nsplit <= _stages(B, H, W)
    x, g = _operands(B, H, W, dev, B * 100 + H + W)
    ref_w, ref_b = _wgrad_reference(x, g)
    runs = []
    for _ in range(2):
        part, bpart = _ww_launch(g, x, nsplit, True, dev)
        dw, db = nan_out(128 * 128 * 9, dev), nan_out(128, dev)
        _ww_reduce(part, nsplit, dw, 128, 0, 0, bpart, db)
        runs.append((part.cpu(), bpart.cpu(), dw.cpu((128, 128, 3, 3)), db.cpu()))
    assert all(same_bits(a, b) for a, b in zip(*runs))
    assert bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][1]).all())       # every partial is written
    name = "wgrad_wino B=%d %dx%d nsplit=%d" % (B, H, W, nsplit)
    vs_aten(name + " dW", runs[0][2], _emulation(x, g), ref_w)
    vs_aten(name + " db", runs[0][3], g.cpu().sum((0, 1, 2)), ref_b)
    nb, _ = _ww_launch(g, x, nsplit, False, dev)                            # without the bias partials: the same sums
    assert same_bits(nb.cpu(), runs[0][0])


def test_wgrad_wino_reduce_column_windows_accumulate_and_bias():
    dev = _gpu()
    from test_gpu_r3 import _wgrad_reference
    B, H, W, nsplit = 3, 13, 37, 9
    x, g = _operands(B, H, W, dev, 77)
    ref_w, ref_b = _wgrad_reference(x, g)
    emul, asum = _emulation(x, g), g.cpu().sum((0, 1, 2))
    part, bpart = _ww_launch(g, x, nsplit, True, dev)
    torch.manual_seed(78)
    base, dbase = torch.randn(128, 288, 3, 3), torch.randn(128)
    for k0 in (0, 80, 160):
        for acc in (0, 1):
            for bias in (0, 1):
                dw, db = nan_out(base.numel(), dev, base), nan_out(128, dev, dbase)
                _ww_reduce(part, nsplit, dw, 288, k0, acc, bpart if bias else None, db if bias else None)
                gw, gb = dw.cpu(base.shape), db.cpu()
                win = base[:, k0:k0 + 128]
                name = "wgrad_wino_reduce k0=%d acc=%d bias=%d" % (k0, acc, bias)
                vs_aten(name + " dW", gw[:, k0:k0 + 128], emul + win if acc else emul, ref_w + win.double() if acc else ref_w)
                assert same_bits(gw[:, :k0], base[:, :k0]) and same_bits(gw[:, k0 + 128:], base[:, k0 + 128:]), name
                if bias:
                    vs_aten(name + " db", gb, asum + dbase if acc else asum, ref_b + dbase.double() if acc else ref_b)
                else:
                    assert same_bits(gb, dbase), name


@pytest.mark.parametrize("nseg", [1, 2, 5, 8])
def test_wgrad_wino_multi_vs_float64_and_the_concatenated_operands(nseg):
    dev = _gpu()
    from bmc_hip import lib, ops
    from test_gpu_r3 import _wgrad_reference
    batches = [1, 3, 1, 2, 1, 1, 2, 1][:nseg]
    H, W = 7, 33
    torch.manual_seed(90 + nseg)
    xs = [torch.randn(b, H, W, 128, device=dev) for b in batches]           # every operand its own allocation
    gs = [torch.randn(b, H, W, 128, device=dev) for b in batches]
    nsplit = min(_stages(sum(batches), H, W), 11)                           # split ranges cross images and segments
    part, bpart = nan_out(nsplit * 16 * 128 * 128, dev), nan_out(nsplit * 128, dev)
    A = (lib.Src * nseg)(*[ops._src(t, 0, 128, 0, None, 0, b) for t, b in zip(gs, batches)])
    X = (lib.Src * nseg)(*[ops._src(t, 0, 128, 0, None, 0, b) for t, b in zip(xs, batches)])
    call("_ww_multi", "bmc_wgrad_wino_multi", A, X, (C.c_int * nseg)(*batches), nseg, H, W, nsplit, part.ptr(), bpart.ptr())
    xc, gc = torch.cat(xs), torch.cat(gs)
    part1, bpart1 = _ww_launch(gc, xc, nsplit, True, dev)
    # the segment table only selects base pointers: the same loads, the same order, the same sums
    assert same_bits(part.cpu(), part1.cpu()) and same_bits(bpart.cpu(), bpart1.cpu())
    dw, db = nan_out(128 * 128 * 9, dev), nan_out(128, dev)
    _ww_reduce(part, nsplit, dw, 128, 0, 0, bpart, db)
    ref_w, ref_b = _wgrad_reference(xc, gc)                                 # float64 over all segments
    name = "wgrad_wino_multi nseg=%d nsplit=%d" % (nseg, nsplit)
    vs_aten(name + " dW", dw.cpu((128, 128, 3, 3)), _emulation(xc, gc), ref_w)
    vs_aten(name + " db", db.cpu(), gc.cpu().sum((0, 1, 2)), ref_b)


@pytest.mark.parametrize("nsplit", [1, 7, 8, 9, 64])
def test_wgrad_wino_reduce_alone_bit_exact_on_integers(nsplit):
    """Synthetic partials 4 x integers: the sums over the splits, the halves of G and their products stay integers."""
    dev = _gpu()
    g = torch.Generator().manual_seed(nsplit)
    part = (4 * torch.randint(-8, 9, (nsplit, 16, 128, 128), generator=g)).float()
    bpart = torch.randint(-64, 65, (nsplit, 128), generator=g).float()
    prior, prior_b = _prior(True, (128, 160, 3, 3), 3), _prior(True, (128,), 4)
    pd, bd = part.to(dev), bpart.to(dev)
    k0 = 16
    for acc in (0, 1):
        for bias in (0, 1):
            init, init_b = prior.clone(), prior_b.clone()
            if not acc:
                init[:, k0:k0 + 128] = NAN
                init_b[:] = NAN
            dw, db = nan_out(init.numel(), dev, init), nan_out(128, dev, init_b)
            _ww_reduce(pd, nsplit, dw, 160, k0, acc, bd if bias else None, db if bias else None)
            rw, rb = R.wino_wgrad_reduce(part, nsplit, init, 160, k0, acc, bpart if bias else None, init_b)
            gw, gb = dw.cpu(init.shape), db.cpu()
            assert torch.equal(gw.double(), rw), (acc, bias)
            assert same_bits(gw[:, :k0], prior[:, :k0]) and same_bits(gw[:, k0 + 128:], prior[:, k0 + 128:])
            assert torch.equal(gb.double(), rb) if bias else same_bits(gb, init_b), (acc, bias)


def test_wgrad_wino_refuses():
    dev = _gpu()
    from bmc_hip import lib, ops
    B, H, W = 2, 5, 17                                                      # 8 stages
    x, g = _operands(B, H, W, dev, 1)
    wide = torch.randn(B, H, W, 256, device=dev)
    part, bpart = Guarded(16 * 128 * 128, dev), Guarded(128, dev)
    src = lambda t, nch=128: ops._src(t, 0, nch, 0, None, 0, B)
    one = lambda a, b, nsplit: (C.byref(a), C.byref(b), B, H, W, nsplit, part.ptr(), bpart.ptr())
    refused("_ww", "bmc_wgrad_wino", *one(src(g), src(x), 0), match="nsplit must be in")
    refused("_ww", "bmc_wgrad_wino", *one(src(g), src(x), _stages(B, H, W) + 1), match="nsplit must be in")
    refused("_ww", "bmc_wgrad_wino", *one(src(g, 64), src(x), 1), match="128-channel windows")
    refused("_ww", "bmc_wgrad_wino", *one(src(g), src(x, 64), 1), match="128-channel windows")
    refused("_ww", "bmc_wgrad_wino", *one(src(g), src(wide), 1), match="pix_stride 128")
    refused("_ww", "bmc_wgrad_wino", *one(src(wide), src(x), 1), match="pix_stride 128")
    refused("_ww", "bmc_wgrad_wino", C.byref(src(g)), C.byref(src(x)), 0, H, W, 1, part.ptr(), bpart.ptr(), match="null argument")
    A, X = (lib.Src * 9)(*[src(g)] * 9), (lib.Src * 9)(*[src(x)] * 9)
    for nseg in (0, 9):
        refused("_ww_multi", "bmc_wgrad_wino_multi", A, X, (C.c_int * 9)(*[B] * 9), nseg, H, W, 1, part.ptr(), bpart.ptr(),
                match="operand pairs per launch")
    refused("_ww_multi", "bmc_wgrad_wino_multi", A, X, (C.c_int * 9)(B, 0, B, B, B, B, B, B, B), 2, H, W, 1, part.ptr(), bpart.ptr(),
            match="empty segment 1")
    assert part.untouched() and bpart.untouched()


def test_wgrad_wino_reduce_refuses():
    dev = _gpu()
    part = torch.ones(16 * 128 * 128, device=dev)
    bpart = torch.ones(128, device=dev)
    dw, db = Guarded(128 * 160 * 9, dev), Guarded(128, dev)
    p = part.data_ptr()
    refused("_ww_red", "bmc_wgrad_wino_reduce", p, 1, dw.ptr(), 64, 0, 0, None, None, match="must lie inside the 64 input")
    refused("_ww_red", "bmc_wgrad_wino_reduce", p, 1, dw.ptr(), 160, 33, 0, None, None, match="must lie inside the 160 input")
    refused("_ww_red", "bmc_wgrad_wino_reduce", p, 1, dw.ptr(), 160, -1, 0, None, None, match="must lie inside")
    refused("_ww_red", "bmc_wgrad_wino_reduce", p, 1, dw.ptr(), 160, 0, 0, bpart.data_ptr(), None, match="bias_part and db go together")
    refused("_ww_red", "bmc_wgrad_wino_reduce", p, 1, dw.ptr(), 160, 0, 0, None, db.ptr(), match="bias_part and db go together")
    refused("_ww_red", "bmc_wgrad_wino_reduce", p, 0, dw.ptr(), 160, 0, 0, None, None, match="bad arguments")
    assert dw.untouched() and db.untouched()
