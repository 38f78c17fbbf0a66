"""chain_kernel<NT, fwd> and chain_kernel<NT, bwd> of csrc/chain.hip (the entry points bmc_chain_fwd / bmc_chain_bwd) alone
against their float64 restatement (tests/chain_ref.py, written from the header's contract and cross-checked against autograd in
tests/test_chain_ref_cpu.py), ELEMENTWISE, every output: yhat, rstd, centre; dz, ds1, ds0.

The arguments are filled as bmc_hip/bie.py fills them: weight streams from bie._chain_streams (the pack kernels under it are
tested bit for bit in test_gpu_weight_path_kernels.py), source descriptors from ops._src, outputs in sentinel-guarded buffers.

Pass rule, per output tensor and case:
  (a) every element: |kernel - float64| <= hard bound (chain_ref.hard_bound_*: first-order running error bound of any fp32
      evaluation of the contract's formulas);
  (b) the kernel's largest elementwise error <= 4 x max(ATen-fp32 error, serial-fp32 error, 1 ulp of the largest output
      magnitude), both yardsticks (chain_ref.chain_fwd / chain_bwd in float32, order "aten" / "serial") measured against the
      same float64 reference on the same inputs; `ratio` below is that quotient;
  (c) on the plain-randn families, whole-tensor rel-L2 < 2e-5 (forward) / 5e-5 (gradients): the bars of test_gpu_r2.py;
  (d) guards intact, two runs bit-identical.
Without a tolerance: a NaN / Inf in one pixel changes no bit of any other pixel (an interior pixel, and the bottom-right pixel
of a ragged image that the clamped loader lanes re-read); identical images at different positions of a many-tiles-per-workgroup
launch give identical bits; bad arguments are refused before anything runs.

Launch arithmetic the shapes come from (csrc/chain.hip, csrc/tile_walk.h): workgroup tile = 4 rows x 16 pixels, all channels;
units = batches (backward: pairs) x ceil(H / 4) x ceil(W / 16); grid = min(units, 2 x CUs); XCD map (eighths of the unit list)
when the grid is a multiple of 8 and units >= grid.
  1x1     every loader lane clamped          3x5    one ragged tile          4x16   exactly one full tile
  5x17    four tiles, three ragged           9x33, 3 batches   27 units: grid not a multiple of 8, the plain map
  19x213, 19 batches   1330 units: at 256 CUs (grid 512) every workgroup walks 2 or 3 units, the eighths have 166 or 167
In backward "batches" is the pair count n: dcentre holds 2n images.

Input families (chain_ref.fwd_inputs / bwd_inputs): plain randn at the parameter scales of the BIE test; lowvar (s0, s1, bf
scaled by 1e-3: variance ~ eps); mean1e3 (bf + 1e3); const (z exact and constant over channels: yhat == 0 exactly, rstd within
1 ulp of 1/sqrtf(eps)); backward with yhat / rstd from the float64 forward rounded to fp32, and synthetic with rstd up to 1e3.
Source forms: contiguous; the production twin maps (s0: mod = n, s1: shift = n, mod = 2n); a channel window c0 = 16 of a
tensor 48 channels wider with b0 = 1 (everything outside the window is NaN); ds0_add absent / contiguous / such a window.

Measured on an MI355X (256 CUs): every `RATIO` line that judge prints (pytest -s), 351 comparisons in all; per output the number
of comparisons, the largest ratio under rule (b), the largest error / hard bound under rule (a), and the case that has each.
The bar of rule (b) is 4, that of rule (a) is 1.

RATIO_TABLE_BEGIN
output  cases  max ratio  at                                                    max err/bound  at
yhat       50       1.96  fwd C=32 1x1 B=2 plain twin                                  0.0537  fwd C=32 5x17 B=2 mean1e3 twin
rstd       50       1.06  fwd C=32 5x17 B=2 plain window                               0.0090  fwd C=32 5x17 B=2 mean1e3 twin
centre     56       1.43  fwd C=32 5x17 B=2 const twin                                 0.0088  fwd C=32 5x17 B=2 mean1e3 twin
dz         65       1.45  bwd C=64 9x33 n=3 fwd dc=contiguous add=absent               0.0683  bwd C=32 19x213 n=19 fwd dc=window add=contiguous walk
ds1        65       1.50  bwd C=32 3x5 n=1 fwd dc=contiguous add=contiguous            0.0147  bwd C=32 19x213 n=19 fwd dc=window add=contiguous walk
ds0        65       1.25  bwd C=32 5x17 n=2 fwd dc=window add=window                   0.0171  bwd C=32 19x213 n=19 fwd dc=window add=contiguous walk

cases with ratio >= 2: none.  (The const family's yhat and rstd are held to exact statements instead of rule (b): yhat == 0,
rstd within 1 ulp of 1/sqrtf(eps); both hold at every C.)  No kernel finding: chain.hip is unchanged.

That the file bites, shown once with five scratch builds of the library, each with one arithmetic-only edit to chain.hip (no
address changes), this file alone run against each:
  a.eps not added                        35 tests fail, e.g. test_fwd_input_families_vs_float64[32-lowvar-5-17-2-twin]: yhat ratio 1.4e6
                                         (plain inputs: rstd ratio 4.65 .. 6.81 at C = 32 -- near the bar, as eps/(2 var) = 4 ulp
                                         predicts; the lowvar and const families are what catches it at every C)
  1.f / (C + 1) in the forward mean      56 fail, e.g. test_fwd_shapes_vs_float64[32-3-5-1-contiguous]: yhat ratio 18699
  m1 not subtracted in backward          65 fail, e.g. test_bwd_shapes_vs_float64[32-3-5-1-contiguous-contiguous]: dz ratio 7.0e5
  Rz[t] += Ra[t] removed                 73 fail, e.g. test_bwd_shapes_vs_float64[32-1-1-1-contiguous-contiguous]: ds0 ratio 2.8e6
  the ds0_add load skipped               50 fail, e.g. test_bwd_shapes_vs_float64[32-1-1-1-contiguous-contiguous]: ds0 ratio 3.0e6
RATIO_TABLE_END
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import chain_ref as R
from test_gpu_r2 import _gpu, _restore_math_mode, rel_l2  # noqa: F401
from test_gpu_streaming_kernels import Guarded, call, refused

pytestmark = pytest.mark.gpu
F32 = torch.float32
EPS = R.EPS
WIDE, C0, B0 = 48, 16, 1          # the channel-window form: a tensor WIDE channels wider, window at c0 = C0, batch offset B0
SHAPES = [(1, 1), (3, 5), (4, 16), (5, 17)]
CS = [32, 64, 128]
WALK = (19, 213, 19)              # H, W, launch batches (backward: pairs)
TH, TW = 4, 16
FWD_OUT, BWD_OUT = ("yhat", "rstd", "centre"), ("dz", "ds1", "ds0")


# ------------------------------------------------------------------ helpers
def _seed(*k):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(k)) % (2 ** 31)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _place(t, form, dev):
    """logical [nb,H,W,C] -> (device tensor, c0, b0): as it is, or as a window of a wider NaN-filled tensor."""
    if form != "window":
        return t.to(dev).contiguous(), 0, 0
    nb, H, W, C = t.shape
    wide = torch.full((nb + B0, H, W, C + WIDE), float("nan"))
    wide[B0:, :, :, C0:C0 + C] = t
    return wide.to(dev), C0, B0


def _desc(t, c0, b0, C, launch_b, shift=0, mod=None):
    from bmc_hip import ops
    return ops._src(t, c0, C, shift, mod, b0, launch_b)


def judge(name, got, ref, bound, aten, serial, l2_bar=None):
    """Rules (a), (b) and, with l2_bar, (c) for one output tensor; prints the RATIO line first."""
    got = got.detach().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    ratio, ke, ae, se, floor = R.rule_b(got, ref, aten, serial)
    err = (got.double() - ref).abs()
    frac = float((err / bound.clamp_min(1e-300)).max())
    print("RATIO %s kernel=%.3e aten=%.3e serial=%.3e ulp=%.3e ratio=%.2f bound=%.4f" % (name, ke, ae, se, floor, ratio, frac))
    assert bool(torch.isfinite(got).all()), name
    assert bool((err <= bound).all()), (name, "hard bound", frac)
    assert ratio <= 4.0, (name, ke, ae, se, floor, ratio)
    if l2_bar is not None:
        l2 = rel_l2(got, ref)
        assert l2 < l2_bar, (name, "rel-L2", l2)
    return ratio


def _walk_counts(nunits, cus):
    """Units per workgroup, the arithmetic of csrc/tile_walk.h at grid = min(units, 2 x CUs)."""
    grid = min(nunits, 2 * cus)
    xcd_map = grid % 8 == 0 and nunits >= grid
    counts = []
    for blk in range(grid):
        if xcd_map:
            xcd, xj, stride = blk % 8, blk // 8, grid // 8
            first, hi = nunits * xcd // 8 + xj, nunits * (xcd + 1) // 8
        else:
            first, hi, stride = blk, nunits, grid
        counts.append((hi - first + stride - 1) // stride if first < hi else 0)
    return grid, counts


def _need_many_tiles_per_workgroup(dev):
    H, W, B = WALK
    nunits = B * -(-H // TH) * -(-W // TW)
    assert nunits == 1330
    grid, counts = _walk_counts(nunits, torch.cuda.get_device_properties(dev).multi_processor_count)
    if not (min(counts) >= 2 and len(set(counts)) > 1):
        pytest.skip("this device gives the %d units to %d workgroups, %d .. %d each: not the walk this case is about"
                    % (nunits, grid, min(counts), max(counts)))
    assert grid % 8 == 0                                             # the XCD map: eighths of unequal size
    assert len({nunits * (x + 1) // 8 - nunits * x // 8 for x in range(8)}) > 1


# ------------------------------------------------------------------ forward: cases, launch, check
def _fwd_maps(form, B):
    """(batches of the s0 tensor, of the s1 tensor, s0's (shift, mod), s1's (shift, mod))."""
    if form == "twin":
        assert B % 2 == 0
        n = B // 2
        return n, B, (0, n), (n, B)
    return B, B, (0, None), (0, None)


def _fwd_logical(C, B, H, W, family, form):
    nb0, nb1, m0, m1 = _fwd_maps(form, B)
    s0, s1, p = R.fwd_inputs(C, nb0, nb1, H, W, family, _seed(C, B, H, W, R.FWD_FAMILIES.index(family), len(form)))
    return s0, s1, p, m0, m1


def _fwd_refs(s0, s1, p, m0, m1, B):
    g0, g1 = R.launch_batches(s0, B, *m0), R.launch_batches(s1, B, *m1)
    args = (g0, g1, p["Wf"], p["bf"], p["gamma"], p["beta"], p["Wc"], p["bc"], EPS)
    return dict(ref=R.chain_fwd(*args), bound=R.hard_bound_fwd(*args), aten=R.chain_fwd(*args, dtype=F32, order="aten"),
                serial=R.chain_fwd(*args, dtype=F32, order="serial"))


@functools.lru_cache(maxsize=None)
def _fwd_case(C, B, H, W, family, form):
    """CPU side of a small forward case, computed once and shared (never modified)."""
    s0, s1, p, m0, m1 = _fwd_logical(C, B, H, W, family, form)
    k = _fwd_refs(s0, s1, p, m0, m1, B)
    k.update(s0=s0, s1=s1, p=p, m0=m0, m1=m1)
    return k


class FwdLaunch:
    """bmc_chain_fwd with its arguments filled as bie.chain_fwd fills them; outputs guarded."""

    def __init__(self, dev, C, B, H, W, s0, s1, p, m0, m1, form):
        from bmc_hip import bie, lib
        self.dev, self.shape = dev, (B, H, W, C)
        self.P = {k: v.to(dev).contiguous() for k, v in p.items()}
        self.t0, c00, b00 = _place(s0, form, dev)
        self.t1, c01, b01 = _place(s1, form, dev)
        self.stream, _ = bie._chain_streams(self.P["Wf"], self.P["Wc"], C)
        a = lib.ChainFwdArgs()
        a.s0, a.s1 = _desc(self.t0, c00, b00, C, B, *m0), _desc(self.t1, c01, b01, C, B, *m1)
        a.wstream = self.stream.data_ptr()
        a.bias_f, a.bias_c = self.P["bf"].data_ptr(), self.P["bc"].data_ptr()
        a.gamma, a.beta = self.P["gamma"].data_ptr(), self.P["beta"].data_ptr()
        a.eps = EPS
        a.B, a.C, a.H, a.W = B, C, H, W
        self.a = a

    def run(self):
        B, H, W, C = self.shape
        n = B * H * W
        yhat, rstd, centre = Guarded(n * C, self.dev), Guarded(n, self.dev), Guarded(n * C, self.dev)
        self.a.yhat, self.a.rstd, self.a.centre = yhat.ptr(), rstd.ptr(), centre.ptr()
        call("_chain_fwd", "bmc_chain_fwd", ctypes.byref(self.a))
        return yhat.cpu((B, H, W, C)), rstd.cpu((B, H, W)), centre.cpu((B, H, W, C))      # .cpu() checks the guards


def _check_fwd(tag, got, k, family):
    plain = family == "plain"
    for i, name in enumerate(FWD_OUT):
        if family == "const" and name != "centre":
            err = (got[i].double() - k["ref"][i]).abs()
            assert bool((err <= k["bound"][i]).all()), (tag, name, "hard bound")
            continue
        judge("%s %s" % (tag, name), got[i], k["ref"][i], k["bound"][i], k["aten"][i], k["serial"][i], 2e-5 if plain else None)
    if family == "const":
        assert bool((got[0] == 0).all()), "yhat of constant rows is exactly 0"
        want = np.float32(1.0) / np.sqrt(np.float32(EPS))
        assert float((got[1] - float(want)).abs().max()) <= float(np.spacing(want)), "rstd within 1 ulp of 1/sqrtf(eps)"
        assert bool((k["ref"][0] == 0).all())                                 # the float64 centre is Wc beta + bc


def _fwd(C, B, H, W, family, form):
    dev = _gpu()
    k = _fwd_case(C, B, H, W, family, form)
    L = FwdLaunch(dev, C, B, H, W, k["s0"], k["s1"], k["p"], k["m0"], k["m1"], form)
    got = L.run()
    _check_fwd("fwd C=%d %dx%d B=%d %s %s" % (C, H, W, B, family, form), got, k, family)
    again = L.run()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again))   # run-to-run identical
    return L, got


FWD_SHAPE_CASES = [(H, W, B, form) for H, W in SHAPES for B, form in ((1, "contiguous"), (2, "twin"))] + [(9, 33, 3, "window")]


@pytest.mark.parametrize("H,W,B,form", FWD_SHAPE_CASES)
@pytest.mark.parametrize("C", CS)
def test_fwd_shapes_vs_float64(C, H, W, B, form):
    _fwd(C, B, H, W, "plain", form)


@pytest.mark.parametrize("H,W,B,form", [(5, 17, 2, "twin"), (4, 16, 1, "window")])
@pytest.mark.parametrize("family", ["lowvar", "mean1e3", "const"])
@pytest.mark.parametrize("C", CS)
def test_fwd_input_families_vs_float64(C, family, H, W, B, form):
    _fwd(C, B, H, W, family, form)


@pytest.mark.parametrize("form", ["contiguous", "twin", "window"])
@pytest.mark.parametrize("C", CS)
def test_fwd_source_forms_vs_float64(C, form):
    _fwd(C, 2, 5, 17, "plain", form)


@pytest.mark.parametrize("C,form", [(32, "window"), (128, "contiguous")])
def test_fwd_many_tiles_per_workgroup(C, form):
    """19 x 213 x 19 batches: every workgroup walks 2 or 3 units, so the load pipeline crosses tile boundaries.  Images 0, 7
    and 18 are identical and sit at different positions of different workgroups' walks: their outputs are bit-identical."""
    dev = _gpu()
    _need_many_tiles_per_workgroup(dev)
    H, W, B = WALK
    s0, s1, p, m0, m1 = _fwd_logical(C, B, H, W, "plain", form)
    for t in (s0, s1):
        t[7] = t[0]
        t[18] = t[0]
    k = _fwd_refs(s0, s1, p, m0, m1, B)
    L = FwdLaunch(dev, C, B, H, W, s0, s1, p, m0, m1, form)
    got = L.run()
    _check_fwd("fwd C=%d %dx%d B=%d plain %s walk" % (C, H, W, B, form), got, k, "plain")
    for t in got:
        assert torch.equal(_bits(t[7]), _bits(t[0])) and torch.equal(_bits(t[18]), _bits(t[0]))
    again = L.run()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again))


@pytest.mark.parametrize("where", ["interior", "bottom_right"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("C", [32, 128])
def test_fwd_nonfinite_pixel_stays_in_its_column(C, value, where):
    """5 x 17: the bottom-right pixel (4, 16) is the one every clamped loader lane of three ragged tiles re-reads."""
    dev = _gpu()
    B, H, W = 2, 5, 17
    k = _fwd_case(C, B, H, W, "plain", "contiguous")
    clean = FwdLaunch(dev, C, B, H, W, k["s0"], k["s1"], k["p"], k["m0"], k["m1"], "contiguous").run()
    b, y, x = (1, 2, 7) if where == "interior" else (1, H - 1, W - 1)
    s0 = k["s0"].clone()
    s0[b, y, x, C // 2 + 1] = value
    bad = FwdLaunch(dev, C, B, H, W, s0, k["s1"], k["p"], k["m0"], k["m1"], "contiguous").run()
    for name, c, d in zip(FWD_OUT, clean, bad):
        assert not bool(torch.isfinite(d[b, y, x]).any()), name               # the value really was read
        same = _bits(c) == _bits(d)
        same[b, y, x] = True
        assert bool(same.all()), name


def _fwd_valid(dev, C=32, B=2, H=3, W=5):
    k = _fwd_case(C, B, H, W, "plain", "contiguous")
    L = FwdLaunch(dev, C, B, H, W, k["s0"], k["s1"], k["p"], k["m0"], k["m1"], "contiguous")
    n = B * H * W
    outs = [Guarded(n * C, dev), Guarded(n, dev), Guarded(n * C, dev)]
    L.a.yhat, L.a.rstd, L.a.centre = (o.ptr() for o in outs)
    return L, outs


def test_fwd_refuses():
    dev = _gpu()
    from bmc_hip import lib, ops
    L, outs = _fwd_valid(dev)
    a = L.a

    def no(**change):
        """One launch with the given fields changed ('s0.ptr' style names reach into a source), then restored."""
        saved = {}
        for key, v in change.items():
            obj, _, f = key.replace("__", ".").rpartition(".")
            obj = getattr(a, obj) if obj else a
            saved[key] = (obj, f, getattr(obj, f))
            setattr(obj, f, v)
        try:
            refused("_chain_fwd", "bmc_chain_fwd", ctypes.byref(a))
        finally:
            for obj, f, v in saved.values():
                setattr(obj, f, v)

    for C in (16, 48):
        no(C=C, s0__nch=C, s1__nch=C)
    for f in ("B", "H", "W"):
        no(**{f: 0})
    for f in ("s0__ptr", "s1__ptr", "wstream", "bias_f", "bias_c", "gamma", "beta", "yhat", "rstd", "centre"):
        no(**{f: None})
    for s in ("s0", "s1"):
        no(**{s + "__nch": 16})
        no(**{s + "__ptr": getattr(a, s).ptr + 4})
        no(**{s + "__pix_stride": 34})
    with pytest.raises(RuntimeError, match="bmc_chain_fwd"):
        lib.call(lib._chain_fwd, "bmc_chain_fwd", None, ops._stream())
    assert all(o.untouched() for o in outs)
    call("_chain_fwd", "bmc_chain_fwd", ctypes.byref(a))                      # and the unchanged arguments do launch
    assert not any(o.untouched() for o in outs)
    for o in outs:
        o.cpu()


# ------------------------------------------------------------------ backward: cases, launch, check
def _bwd_refs(dc, yhat, rstd, add, p, n):
    args = (dc, yhat, rstd, p["gamma"], p["Wf"], p["Wc"], add, n)
    return dict(ref=R.chain_bwd(*args), bound=R.hard_bound_bwd(*args), aten=R.chain_bwd(*args, dtype=F32, order="aten"),
                serial=R.chain_bwd(*args, dtype=F32, order="serial"))


@functools.lru_cache(maxsize=None)
def _bwd_case(C, n, H, W, family, with_add):
    dc, yhat, rstd, add, p = R.bwd_inputs(C, n, H, W, family, _seed(C, n, H, W, R.BWD_FAMILIES.index(family)))
    add = add if with_add else None
    k = _bwd_refs(dc, yhat, rstd, add, p, n)
    k.update(dc=dc, yhat=yhat, rstd=rstd, add=add, p=p)
    return k


class BwdLaunch:
    """bmc_chain_bwd with its arguments filled as bie.chain_bwd fills them; dz, ds1 (preallocated) and ds0 guarded."""

    def __init__(self, dev, C, n, H, W, dc, yhat, rstd, add, p, dc_form, add_form):
        from bmc_hip import bie, lib, ops
        assert (add is None) == (add_form == "absent")
        self.dev, self.shape = dev, (n, H, W, C)
        self.P = {k: v.to(dev).contiguous() for k, v in p.items()}
        self.tdc, c0, b0 = _place(dc, dc_form, dev)
        self.yhat, self.rstd = yhat.to(dev).contiguous(), rstd.to(dev).contiguous()
        _, self.stream = bie._chain_streams(self.P["Wf"], self.P["Wc"], C)
        a = lib.ChainBwdArgs()
        a.dcentre = _desc(self.tdc, c0, b0, C, 2 * n)
        a.wstream = self.stream.data_ptr()
        a.gamma, a.yhat, a.rstd = self.P["gamma"].data_ptr(), self.yhat.data_ptr(), self.rstd.data_ptr()
        if add is None:
            a.ds0_add = ops._null_src()
        else:
            self.tadd, ca, ba = _place(add, add_form, dev)
            a.ds0_add = _desc(self.tadd, ca, ba, C, n)
        a.n, a.C, a.H, a.W = n, C, H, W
        self.a = a

    def run(self):
        n, H, W, C = self.shape
        px = H * W * C
        dz, ds1, ds0 = Guarded(2 * n * px, self.dev), Guarded(2 * n * px, self.dev), Guarded(n * px, self.dev)
        self.a.dz, self.a.ds1, self.a.ds0 = dz.ptr(), ds1.ptr(), ds0.ptr()
        call("_chain_bwd", "bmc_chain_bwd", ctypes.byref(self.a))
        return dz.cpu((2 * n, H, W, C)), ds1.cpu((2 * n, H, W, C)), ds0.cpu((n, H, W, C))


def _check_bwd(tag, got, k, plain):
    for i, name in enumerate(BWD_OUT):
        judge("%s %s" % (tag, name), got[i], k["ref"][i], k["bound"][i], k["aten"][i], k["serial"][i], 5e-5 if plain else None)


def _bwd(C, n, H, W, family, dc_form, add_form):
    dev = _gpu()
    k = _bwd_case(C, n, H, W, family, add_form != "absent")
    L = BwdLaunch(dev, C, n, H, W, k["dc"], k["yhat"], k["rstd"], k["add"], k["p"], dc_form, add_form)
    got = L.run()
    _check_bwd("bwd C=%d %dx%d n=%d %s dc=%s add=%s" % (C, H, W, n, family, dc_form, add_form), got, k, family == "fwd")
    again = L.run()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again))
    return L, got


BWD_SHAPE_CASES = [(H, W, n, dcf, addf) for H, W in SHAPES
                   for n, dcf, addf in ((1, "contiguous", "contiguous"), (2, "window", "window"))] + \
    [(9, 33, 3, "contiguous", "absent")]


@pytest.mark.parametrize("H,W,n,dc_form,add_form", BWD_SHAPE_CASES)
@pytest.mark.parametrize("C", CS)
def test_bwd_shapes_vs_float64(C, H, W, n, dc_form, add_form):
    _bwd(C, n, H, W, "fwd", dc_form, add_form)


# n runs against the add form the other way round than in the shape cases: absent at n = 1, contiguous at 2, a window at 3
@pytest.mark.parametrize("family", R.BWD_FAMILIES)
@pytest.mark.parametrize("n,add_form", [(1, "absent"), (2, "contiguous"), (3, "window")])
@pytest.mark.parametrize("dc_form", ["contiguous", "window"])
@pytest.mark.parametrize("C", CS)
def test_bwd_forms_and_saved_state_vs_float64(C, dc_form, n, add_form, family):
    _bwd(C, n, 5, 17, family, dc_form, add_form)


@pytest.mark.parametrize("C,dc_form,add_form", [(32, "window", "contiguous"), (128, "contiguous", "window")])
def test_bwd_many_tiles_per_workgroup(C, dc_form, add_form):
    """19 x 213, n = 19 pairs (38 images of dcentre): every workgroup walks 2 or 3 pairs of tiles.  Pairs 0, 7 and 18 are
    identical in all of their operands: their results are bit-identical."""
    dev = _gpu()
    _need_many_tiles_per_workgroup(dev)
    H, W, n = WALK
    dc, yhat, rstd, add, p = R.bwd_inputs(C, n, H, W, "fwd", _seed(C, n, H, W))
    for t in (dc, yhat, rstd):
        for b in (7, 18):
            t[b], t[b + n] = t[0], t[n]
    add[7] = add[0]
    add[18] = add[0]
    k = _bwd_refs(dc, yhat, rstd, add, p, n)
    L = BwdLaunch(dev, C, n, H, W, dc, yhat, rstd, add, p, dc_form, add_form)
    got = L.run()
    _check_bwd("bwd C=%d %dx%d n=%d fwd dc=%s add=%s walk" % (C, H, W, n, dc_form, add_form), got, k, True)
    dz, ds1, ds0 = got
    for b in (7, 18):
        for t in (dz, ds1):
            assert torch.equal(_bits(t[b]), _bits(t[0])) and torch.equal(_bits(t[b + n]), _bits(t[n]))
        assert torch.equal(_bits(ds0[b]), _bits(ds0[0]))
    again = L.run()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again))


@pytest.mark.parametrize("where", ["interior", "bottom_right"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("C", [32, 128])
def test_bwd_nonfinite_pixel_stays_in_its_column(C, value, where):
    dev = _gpu()
    n, H, W = 2, 5, 17
    k = _bwd_case(C, n, H, W, "fwd", True)
    mk = lambda dc: BwdLaunch(dev, C, n, H, W, dc, k["yhat"], k["rstd"], k["add"], k["p"], "contiguous", "contiguous").run()
    clean = mk(k["dc"])
    bb, y, x = (3, 2, 7) if where == "interior" else (3, H - 1, W - 1)
    dc = k["dc"].clone()
    dc[bb, y, x, C // 2 + 1] = value
    bad = mk(dc)
    hit = {"dz": bb, "ds1": (bb + n) % (2 * n), "ds0": bb % n}                # the images the pixel's column reaches
    for name, c, d in zip(BWD_OUT, clean, bad):
        assert not bool(torch.isfinite(d[hit[name], y, x]).any()), name
        same = _bits(c) == _bits(d)
        same[hit[name], y, x] = True
        assert bool(same.all()), name


def test_bwd_refuses():
    dev = _gpu()
    from bmc_hip import lib, ops
    C, n, H, W = 32, 2, 3, 5
    k = _bwd_case(C, n, H, W, "fwd", True)
    L = BwdLaunch(dev, C, n, H, W, k["dc"], k["yhat"], k["rstd"], k["add"], k["p"], "contiguous", "contiguous")
    px = H * W * C
    outs = [Guarded(2 * n * px, dev), Guarded(2 * n * px, dev), Guarded(n * px, dev)]
    a = L.a
    a.dz, a.ds1, a.ds0 = (o.ptr() for o in outs)

    def no(**change):
        saved = {}
        for key, v in change.items():
            obj, _, f = key.replace("__", ".").rpartition(".")
            obj = getattr(a, obj) if obj else a
            saved[key] = (obj, f, getattr(obj, f))
            setattr(obj, f, v)
        try:
            refused("_chain_bwd", "bmc_chain_bwd", ctypes.byref(a))
        finally:
            for obj, f, v in saved.values():
                setattr(obj, f, v)

    for Cbad in (16, 48):
        no(C=Cbad, dcentre__nch=Cbad)
    for f in ("n", "H", "W"):
        no(**{f: 0})
    for f in ("dcentre__ptr", "wstream", "gamma", "yhat", "rstd", "dz", "ds1", "ds0"):
        no(**{f: None})
    no(dcentre__nch=16)
    no(dcentre__ptr=a.dcentre.ptr + 4)
    no(dcentre__pix_stride=34)
    no(ds0_add__ptr=a.ds0_add.ptr + 4)
    no(ds0_add__pix_stride=34)
    with pytest.raises(RuntimeError, match="bmc_chain_bwd"):
        lib.call(lib._chain_bwd, "bmc_chain_bwd", None, ops._stream())
    assert all(o.untouched() for o in outs)
    call("_chain_bwd", "bmc_chain_bwd", ctypes.byref(a))
    assert not any(o.untouched() for o in outs)
    for o in outs:
        o.cpu()
