"""bmc_pgemm alone (csrc/pgemm.hip, csrc/pgemm_bf.hip), every kernel instantiation, against its float64 restatement
(tests/pgemm_ref.py, which tests/test_pgemm_ref_cpu.py ties to F.conv2d's autograd and torch.bmm).

The entry point is called through lib.call with a lib.PgemmArgs this file fills in itself: nsplit and tap_groups are the case's, not
what ops.pgemm_raw would choose, so that the branches the dispatcher never produces are run too (the case table and what each
shape is for: pgemm_ref.SHAPES / pgemm_ref.CASES; that it reaches every instantiation and branch is asserted on the CPU).

Buffers.  `slabs` [nsplit][G][taps][Mpad][Npad] and `bias_slabs` [nsplit][G][4][Mpad] are Guarded buffers with a NaN payload: every
element has to be written, the guards have to survive, pad rows m >= M are 0.0 in both and pad columns n >= N are 0.0 in the slabs
(they are products with the zero buffer).  A split without tiles (nsplit above the tile count) leaves an all-zero slab and all-zero
bias partials.  Every operand is the channel window [4, 4 + nch) of a tensor 8 channels wider, and images [1, 1 + B) of a batch two
images longer; everything outside the window is NaN, so a stray read poisons the sums.  The zero buffer is exactly the 64 bytes the
header asks for, between NaNs.  Table operands are separately allocated images behind a bmc_ptr_table table, as ops._table_src
builds them (batch_stride 0: a kernel that ignored the table would read image 0 throughout).

What is compared: the slabs summed over the splits in float64 on the CPU against C, the bias partials summed over splits and the 4
parts against the bias gradient.  Which tile goes to which split is not part of the header and is not asserted.

Bars, fixed in advance, none measured:
  * integer operands in [-8, 8] (math 0, 1, 3): torch.equal for C and the bias gradient -- every product and partial sum is an
    integer below 2^24, every operand is a bf16 value;
  * randn, math 0: per element |got - ref64| <= n 2^-24 sum |a x|, n = the element's number of in-image products: the order-free
    first-order bound of an fp32 sum (the form of the reductions' bound in test_gpu_weight_path_kernels.py); the bias gradient
    n 2^-24 sum |a|, n = the group's pixels, in every mode (all kernels add up fp32 values of A).  At most 2048 pixels per group, so
    one dropped or doubled product of typical size is above the bound (tests/test_pgemm_ref_cpu.py);
  * randn, math 3: rel-L2 against the unrounded float64 reference < BAR_X6 = 3e-6 (test_gpu_bf16_kernels.py's bar for the mode);
  * math 1 on randn is held by test_gpu_bf16_kernels.py and not repeated;
  * two runs of every case are bit-identical.

The kernels.  The issue behind this file counts 16; the two launchers hold 18 instantiations, and all 18 are reached: the 10
pgemm_dma_kernel ones (<9>, <9,9,true>, <9,3>, <9,3,true>, KS = 2 and 4 with and without tables, <1>, <1,1,true>) and 8 bf16 ones
(pgemm_bf9x3_kernel<false|true>, pgemm_bf_kernel<1,3[,true]>, pgemm_bf_kernel<9,1[,true]>, pgemm_bf_kernel<1,1[,true]>).

Worst err / bound per kernel, as test_zz_ratio_table prints it (pytest -s) after all cases ran on an MI355X.  C and db: randn cases,
error over the bound above (math 3: rel-L2 over BAR_X6 for C); integer cases are exact or fail.  A record, not a bar.

RATIO_TABLE_BEGIN
kernel              worst C err/bound  at                                  worst db err/bound  at
dma<9,9>            0.464              i1-ns3-m0-randn                     0.013               i3-ns2-m0-randn
dma<9,9,tab>        0.004              h-ns7-m0-taba-randn                 0.001               g-ns5-m0-taball-randn
dma<9,3>            0.006              j128x16_9x21-ns3-m0-tg3-randn       0.001               j128x16_9x21-ns3-m0-tg3-randn
dma<9,3,tab>        0.004              h-ns7-m0-taball-tg3-randn           0.001               g-ns5-m0-taball-tg3-randn
dma<9,9,ks2>        0.004              p-ns3-m0-randn                      0.001               j48x32_9x21-ns3-m0-randn
dma<9,9,tab,ks2>    0.004              j128x16_9x21-ns3-m0-taball-randn    0.001               j48x32_9x21-ns3-m0-taball-randn
dma<9,9,ks4>        0.003              j32x256_9x21-ns3-m0-randn           0.001               j32x32_9x21-ns3-m0-randn
dma<9,9,tab,ks4>    0.003              j32x256_9x21-ns3-m0-taball-randn    0.001               j32x32_9x21-ns3-m0-taball-randn
dma<1,1>            0.467              n-ns3-m0-randn                      0.007               o-ns2-m0-randn
dma<1,1,tab>        0.013              b-ns1-m0-taball-randn               0.002               c-ns2-m0-taball-randn
bf9x3               0.065              g-ns5-m3-randn                      0.001               h-ns7-m3-randn
bf9x3<tab>          0.065              g-ns5-m3-taball-randn               0.001               h-ns7-m3-taball-randn
bf<1,3>             0.084              b-ns1-m3-randn                      0.001               b-ns1-m3-randn
bf<1,3,tab>         0.084              b-ns1-m3-taball-randn               0.001               b-ns1-m3-taball-randn
bf<9,1>             (integer cases only)                                      -
bf<9,1,tab>         (integer cases only)                                      -
bf<1,1>             (integer cases only)                                      -
bf<1,1,tab>         (integer cases only)                                      -
RATIO_TABLE_END
(The two ratios near 0.47 are the one-pixel images: n = 2 products, so the bound is two roundings of the sum and the kernel used one.
Everywhere else the fp32 kernels use less than 0.02 of the bound, the bf16x6 ones less than 0.09 of BAR_X6.)

Findings.  All 171 tests passed on the kernels as they were: no kernel and no branch failed a bar.  What the work turned up:
  * bmc_pgemm checked nch % 4 and pix_stride % 4 of every operand, but not what the same 16-byte-per-lane tile fills need beside
    them: LDS-DMA `global_load_lds_dwordx4` in pgemm.hip (csrc/dma_ring.h: dma16, dma16v) and 16-byte global loads through
    `f32x4` pointers in pgemm_bf.hip (ldg16, and global_load_dwordx4 in pgemm_bf9x3_kernel) address
    ptr + 4 (image * batch_stride + pixel * pix_stride + channel quad), which is a multiple of 16 only if ptr and
    4 * batch_stride are; the zero buffer is read the same way.  bmc_conv checks all of this, bmc_pgemm did not.  Every caller
    in bmc_hip passes aligned operands, so nothing was wrong in use; a misaligned launch was NOT run to see what it does.  The
    entry point now refuses a pointer, batch stride or zero buffer that is not 16-byte aligned (a table operand: the table
    itself, 8 bytes; the image pointers inside it are device data and remain the caller's duty), include/bmc_hip.h states the
    requirement, and test_pgemm_refuses holds the refusals;
  * the header said nothing about nsplit above the tile count.  The kernels serve it (zero slab, zero bias partials: cases
    a-ns3, n-ns3, i1-ns3 in all three math modes) and the header now says so;
  * the shapes the issue lists never give a 1x1 split three tiles, so the 1x1 kernels' second use of an LDS buffer (fp32) and the
    refill of the two-tile register ring (bf16) were not run by them: with `load_tile(tile + PD * nsplit, d)` of pgemm_bf_kernel
    changed to reload an earlier tile on a scratch copy, all listed 1x1 cases still passed.  Shapes b-ns1 (6 tiles, one split) and
    r (4 full tiles through the uniform-base path) were added and fail on that copy; tests/test_pgemm_ref_cpu.py asserts that
    each tap count and math mode has such a case;
  * the same scratch copy also had the 3x3 tile walk's carry from tile rows into the image index removed and the bias partials'
    pad rows left unwritten (all three defects only mis-sum or skip writes; none reads or writes out of range): 92 of the 171
    tests here fail on it, while tests/test_gpu_pgemm9_wavemap.py passes on it unchanged;
  * also added beyond the issue's list: bias partials over two row blocks with M < Mpad (o, p: the listed (c) has M = Mpad, (b)
    one row block), BMC_MAX_SRC sources (q1, q9), two groups on 3x3 (m), one-pixel images on 1x1 (n), the tap-row kernel on
    shapes that leave its 4 x 2 map idle waves (j128x16, j32x32 with tap_groups 3), 3x3 with only A a table;
  * NOT run: the `H W pix_stride >= 2^28` exit from the uniform-base fill (32-bit byte offsets) needs an operand above 1 GiB.
"""
import ctypes as C
import re

import pytest
import torch

import pgemm_ref as R
from test_gpu_r2 import _gpu
from test_gpu_streaming_kernels import SENT, Guarded, call, refused  # noqa: F401
from test_gpu_weight_path_kernels import nan_out

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN = float("nan")
BAR_X6 = 3e-6
C0, B0, CPAD = 4, 1, 8          # every operand: channels [C0, C0 + nch) of nch + CPAD, images [B0, B0 + Bt) of Bt + 2

_ZERO = {}
WORST = {}                      # kernel -> {"C": (ratio, case), "db": (ratio, case)}
RAN = set()


def _zeros(dev):
    if dev not in _ZERO:
        z = torch.full((48,), NAN)
        z[16:32] = 0.0
        _ZERO[dev] = z.to(dev)
    return _ZERO[dev].data_ptr() + 64


def _plain(t, shift, mod, launch_b, dev, keep):
    from bmc_hip import lib
    Bt, H, W, n = t.shape
    big = torch.full((Bt + 2, H, W, n + CPAD), NAN)
    big[B0:B0 + Bt, :, :, C0:C0 + n] = t
    big = big.to(dev)
    keep.append(big)
    s = lib.Src()
    s.ptr = big.data_ptr() + 4 * (B0 * H * W * (n + CPAD) + C0)
    s.batch_stride, s.pix_stride, s.nch = H * W * (n + CPAD), n + CPAD, n
    s.batch_shift, s.batch_mod = shift, mod if mod is not None else launch_b
    return s


def _table(t, shift, mod, launch_b, dev, keep):
    from bmc_hip import lib
    _, H, W, n = t.shape
    imgs = []
    for b in range(launch_b):
        img = torch.full((H, W, n + CPAD), NAN)
        img[:, :, C0:C0 + n] = t[(b + shift) % mod if mod is not None else b + shift]
        imgs.append(img.to(dev))
    table = torch.empty(launch_b, dtype=torch.int64, device=dev)
    call("_ptr_table", "bmc_ptr_table", (C.c_ulonglong * launch_b)(*[i.data_ptr() + 4 * C0 for i in imgs]), launch_b, table.data_ptr())
    keep.extend(imgs + [table])
    s = lib.Src()
    s.ptr = table.data_ptr()
    s.batch_stride, s.pix_stride, s.nch, s.batch_shift, s.batch_mod = 0, n + CPAD, n, 0, lib.SRC_TABLE
    return s


def _args(c, dev, slabs_ptr, bias_ptr):
    """The argument block of a case and the tensors it points into."""
    from bmc_hip import lib
    s = R.SHAPES[c.shape]
    a_t, x_ts = R.operands(c.shape, c.data)
    keep = []
    p = lib.PgemmArgs()
    p.a = (_table if c.tab in ("all", "a") else _plain)(a_t, 0, None, s.B, dev, keep)
    p.nsrc = len(x_ts)
    for i, x in enumerate(x_ts):
        p.src[i] = (_table if c.tab == "all" else _plain)(x, s.shift, s.mod, s.B, dev, keep)
    p.B, p.H, p.W, p.taps, p.batch_per_group = s.B, s.H, s.W, s.taps, s.bpg
    p.slabs, p.nsplit, p.zeros, p.bias_slabs = slabs_ptr, c.nsplit, _zeros(dev), bias_ptr
    p.math, p.tap_groups = c.math, c.tap_groups
    return p, keep


def _dims(c):
    s = R.SHAPES[c.shape]
    return s, s.B // s.bpg, s.M, sum(s.widths), R.pad32(s.M), R.pad32(sum(s.widths))


def _launch(c, dev):
    s, G, M, N, Mpad, Npad = _dims(c)
    slabs = nan_out(c.nsplit * G * s.taps * Mpad * Npad, dev)
    bias = nan_out(c.nsplit * G * 4 * Mpad, dev) if s.bias else None
    p, keep = _args(c, dev, slabs.ptr(), bias.ptr() if bias is not None else None)
    call("_pgemm", "bmc_pgemm", C.byref(p))
    out = slabs.cpu((c.nsplit, G, s.taps, Mpad, Npad)), bias.cpu((c.nsplit, G, 4, Mpad)) if bias is not None else None
    del keep
    return out


def _note(kernel, what, ratio, cid):
    w = WORST.setdefault(kernel, {})
    if what not in w or ratio > w[what][0]:
        w[what] = (ratio, cid)


def _bounded(what, got, ref, bound, kernel, cid):
    err = (got - ref).abs()
    inf_or_0 = torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))      # a zero bound admits no error
    ratio = float(torch.where(bound > 0, err / bound.clamp_min(1e-300), inf_or_0).max())
    print("RATIO %-18s %-34s %-2s max err %.3e  err/bound %.3f" % (kernel, cid, what, float(err.max()), ratio))
    _note(kernel, what, ratio, cid)
    assert bool((err <= bound).all()), (cid, what, float(err.max()), ratio)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_pgemm_kernel_vs_float64(c):
    dev = _gpu()
    s, G, M, N, Mpad, Npad = _dims(c)
    cid, kernel = R.case_id(c), R.case_kernel(c)
    ref = R.reference(c.shape, c.data)
    slabs, bias = _launch(c, dev)
    slabs2, bias2 = _launch(c, dev)

    assert bool(torch.isfinite(slabs).all()), "%s: %d slab elements not written (or poisoned)" % (cid, int((~torch.isfinite(slabs)).sum()))
    assert not bool(slabs[:, :, :, M:, :].any()) and not bool(slabs[:, :, :, :, N:].any()), cid + ": pad rows / columns are not 0.0"
    assert torch.equal(slabs.view(torch.int32), slabs2.view(torch.int32)), cid + ": two runs differ"
    if bias is not None:
        assert bool(torch.isfinite(bias).all()), "%s: %d bias partials not written (or poisoned)" % (cid, int((~torch.isfinite(bias)).sum()))
        assert not bool(bias[:, :, :, M:].any()), cid + ": bias pad rows are not 0.0"
        assert torch.equal(bias.view(torch.int32), bias2.view(torch.int32)), cid + ": two runs differ (bias)"
    ntiles = s.bpg * R.tiles_per_image(s)
    if c.nsplit > ntiles:           # splits without tiles: zero slabs, zero bias partials
        empty = [i for i in range(c.nsplit) if not bool(slabs[i].any()) and (bias is None or not bool(bias[i].any()))]
        assert len(empty) >= c.nsplit - ntiles, (cid, empty)

    got = slabs.to(F64).sum(0)[:, :, :M, :N]
    got_b = bias.to(F64).sum((0, 2))[:, :M] if bias is not None else None
    if c.data == "int":
        assert torch.equal(got, ref.C), "%s: %d elements of C differ, max %g" % (cid, int((got != ref.C).sum()), float((got - ref.C).abs().max()))
        if bias is not None:
            assert torch.equal(got_b, ref.db), "%s: bias gradient differs, max %g" % (cid, float((got_b - ref.db).abs().max()))
    else:
        if c.math == 0:
            _bounded("C", got, ref.C, ref.count * R.U32 * ref.absC, kernel, cid)
        else:
            rel = float((got - ref.C).norm() / ref.C.norm())
            print("RATIO %-18s %-34s C  rel-L2 %.3e  err/bound %.3f" % (kernel, cid, rel, rel / BAR_X6))
            _note(kernel, "C", rel / BAR_X6, cid)
            assert rel < BAR_X6, (cid, rel)
        if bias is not None:
            _bounded("db", got_b, ref.db, s.bpg * s.H * s.W * R.U32 * ref.absdb, kernel, cid)
    RAN.add(c)


def test_wave_map_agrees_with_the_restatement():
    _gpu()
    from bmc_hip import lib
    for taps in (1, 9):
        for M in (4, 16, 32, 36, 48, 64, 128, 132, 160):
            for N in (4, 16, 32, 36, 64, 80, 128, 256, 272):
                assert lib.pgemm_wave_map(taps, M, N) == R.wave_map(taps, M, N), (taps, M, N)


def test_pgemm_refuses():
    dev = _gpu()
    from bmc_hip import lib
    c = R.Case("h", 7, 0, "", 1, "int")
    s, G, M, N, Mpad, Npad = _dims(c)
    slabs = Guarded(c.nsplit * G * s.taps * Mpad * Npad, dev)
    bias = Guarded(c.nsplit * G * 4 * Mpad, dev)

    def attempt(msg, mutate, case=c):
        p, keep = _args(case, dev, slabs.ptr(), bias.ptr())
        mutate(p)
        refused("_pgemm", "bmc_pgemm", C.byref(p), match=re.escape(msg))
        torch.cuda.synchronize()
        del keep

    def setter(path, value=None, add=None):
        def mutate(p):
            obj, names = p, path.split(".")
            for nm in names[:-1]:
                obj = obj[int(nm)] if nm.isdigit() else getattr(obj, nm)
            setattr(obj, names[-1], value if add is None else (getattr(obj, names[-1]) or 0) + add)
        return mutate

    refused("_pgemm", "bmc_pgemm", None, match=re.escape("bmc_pgemm: null args"))
    attempt("bmc_pgemm: nsrc=0 out of range", setter("nsrc", 0))
    attempt("bmc_pgemm: nsrc=%d out of range" % (lib.MAX_SRC + 1), setter("nsrc", lib.MAX_SRC + 1))
    attempt("bmc_pgemm: taps must be 1 or 9", setter("taps", 3))
    tg_msg = "bmc_pgemm: tap_groups must be 0, 1, or 3 (3: taps = 9, fp32 or bf16 arithmetic)"
    attempt(tg_msg, lambda p: (setter("taps", 1)(p), setter("tap_groups", 3)(p)))
    attempt(tg_msg, lambda p: (setter("math", 3)(p), setter("tap_groups", 3)(p)))
    attempt(tg_msg, setter("tap_groups", 2))
    attempt("bmc_pgemm: B % batch_per_group != 0", lambda p: (setter("B", 3)(p), setter("batch_per_group", 2)(p)))
    attempt("bmc_pgemm: B % batch_per_group != 0", setter("batch_per_group", 0))
    attempt("bmc_pgemm: nsplit/slabs", setter("nsplit", 0))
    attempt("bmc_pgemm: nsplit/slabs", setter("slabs", None))
    attempt("bmc_pgemm: the zero buffer is required", setter("zeros", None))
    attempt("bmc_pgemm: bad A operand", setter("a.nch", 46))
    attempt("bmc_pgemm: bad A operand", setter("a.pix_stride", add=2))
    attempt("bmc_pgemm: bad A operand", setter("a.ptr", None))
    attempt("bmc_pgemm: bad source 1", setter("src.1.nch", 30))
    attempt("bmc_pgemm: bad source 0", setter("src.0.pix_stride", add=1))
    attempt("bmc_pgemm: bad source 1", setter("src.1.ptr", None))
    attempt("bmc_pgemm: unknown math mode 7", setter("math", 7))
    attempt("bmc_pgemm: unknown math mode 2", setter("math", 2))
    # the tile fills move 16 bytes per lane: pointers and batch strides that are not multiples of 16 bytes
    al = ": pointer and batch stride must be 16-byte aligned"
    attempt("bmc_pgemm: A operand" + al, setter("a.ptr", add=4))
    attempt("bmc_pgemm: A operand" + al, setter("a.batch_stride", add=2))
    attempt("bmc_pgemm: source 1" + al, setter("src.1.ptr", add=8))
    attempt("bmc_pgemm: source 0" + al, setter("src.0.batch_stride", add=1))
    attempt("bmc_pgemm: the zero buffer must be 16-byte aligned", setter("zeros", add=4))
    attempt("bmc_pgemm: A operand" + al, setter("a.ptr", add=4), case=c._replace(tab="a"))      # the table itself: 8 bytes
    for math in (1, 3):             # the bf16 launcher is behind the same checks
        attempt("bmc_pgemm: source 1" + al, setter("src.1.ptr", add=4), case=c._replace(math=math))
    assert slabs.untouched() and bias.untouched()


def test_zz_ratio_table():
    """Prints the record kept in this file's docstring; asserts only that, when every case ran, every kernel was reached."""
    _gpu()
    print("\nkernel              worst C err/bound  at                                  worst db err/bound  at")
    for k in R.ALL_KERNELS:
        w = WORST.get(k, {})
        cr, dbr = w.get("C"), w.get("db")
        print("%-18s  %-17s  %-34s  %-18s  %s" % (k, "%.3f" % cr[0] if cr else "(integer cases only)", cr[1] if cr else "",
                                                   "%.3f" % dbr[0] if dbr else "-", dbr[1] if dbr else ""))
    if len(RAN) == len(R.CASES):
        assert {R.case_kernel(c) for c in RAN} == set(R.ALL_KERNELS)
