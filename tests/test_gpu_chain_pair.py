"""The paired forward of the fused centre chain: chain_kernel<NT, fwd, pair> of csrc/chain.hip, which walks the pixel tile of
launch batch b together with the same tile of batch b + n (n = B / 2) and computes the half of convf that both batches share
(b_f + W_f[:, :C] s0, s0 mapping b and b + n to one image) once.  Every accumulator's MFMA chain is that of the unpaired
kernel, so the paired launch must give the unpaired launch's BITS: torch.equal on yhat, rstd and centre, no tolerance.

BMC_CHAIN_PAIR selects the kernel per launch: 1 = pair, or refuse the call if the launch cannot be paired (that is how these
tests know the paired kernel ran); 0 = never pair; unset = the host's rule (more than one pair per CU, and fewer steps on the
fullest CU: 5 ceil(P / CUs) < 3 ceil(2P / CUs) for P pairs).  The rule is a file-local host function of chain.hip (no export
reaches it), so it is checked through launches: at 5x17 (12 pairs: unpaired by the rule) and at 19x213, n = 19 (paired by the
rule at 256 CUs) the unset switch gives the bits of both forced forms.

Shapes (workgroup tile = 4 rows x 16 pixels): 1x1 every loader lane clamped, 3x5 one ragged tile, 4x16 exactly one tile, 5x17
four tiles of which three ragged; n = 1 and 3; 19x213 with n = 19: 1330 pairs, at 256 CUs every workgroup walks 2 or 3 pairs
and the loaders cross unit boundaries.  Source forms: the production twin map (s0: mod = n, s1: shift = n, mod = 2n) on
contiguous tensors, and through a channel window with a batch offset inside NaN-filled wider tensors.
Against float64 the paired launch is held to the two rules of test_gpu_chain_kernels.py (hard bound; 4 x the fp32
yardsticks): no new tolerance.
"""
import ctypes

import pytest
import torch

import chain_ref as R
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_streaming_kernels import Guarded, call, refused
from test_gpu_chain_kernels import (CS, FWD_OUT, SHAPES, WALK, FwdLaunch, _bits, _check_fwd, _fwd_logical, _fwd_refs,
                                    _need_many_tiles_per_workgroup)

pytestmark = pytest.mark.gpu
SWITCH = "BMC_CHAIN_PAIR"


def _mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, str(mode))


def _run(monkeypatch, L, mode):
    _mode(monkeypatch, mode)
    return L.run()


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _twin_launch(dev, C, n, H, W, family="plain", place="contiguous", edit=None):
    """-> (FwdLaunch over 2n launch batches with the twin maps, its logical inputs); edit(s0, s1) may change them first."""
    B = 2 * n
    s0, s1, p, m0, m1 = _fwd_logical(C, B, H, W, family, "twin")
    if edit is not None:
        edit(s0, s1)
    return FwdLaunch(dev, C, B, H, W, s0, s1, p, m0, m1, place), (s0, s1, p, m0, m1)


# ------------------------------------------------------------------ paired == unpaired, bit for bit
@pytest.mark.parametrize("place", ["contiguous", "window"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("C", CS)
def test_paired_equals_unpaired(monkeypatch, C, H, W, n, place):
    dev = _gpu()
    L, _ = _twin_launch(dev, C, n, H, W, place=place)
    unpaired = _run(monkeypatch, L, 0)
    paired = _run(monkeypatch, L, 1)
    for name, u, q in zip(FWD_OUT, unpaired, paired):
        assert bool(torch.isfinite(u).all()), name
        assert torch.equal(_bits(u), _bits(q)), (name, int((_bits(u) != _bits(q)).sum()))
    assert _same(paired, _run(monkeypatch, L, 1))                             # two paired runs: identical bits


@pytest.mark.parametrize("C,place", [(32, "window"), (128, "contiguous")])
def test_paired_many_pairs_per_workgroup(monkeypatch, C, place):
    """19 x 213, n = 19: 1330 pairs on 512 workgroups.  Images 0, 7 and 18 of xs are identical, and so are the x12 images
    that launch batches 0, 7, 18 (and n + 0, n + 7, n + 18) read: their outputs are bit-identical wherever they sit in a walk."""
    dev = _gpu()
    _need_many_tiles_per_workgroup(dev)
    H, W, n = WALK

    def edit(s0, s1):
        for b in (7, 18):
            s0[b] = s0[0]
            s1[b], s1[b + n] = s1[0], s1[n]
    L, _ = _twin_launch(dev, C, n, H, W, place=place, edit=edit)
    unpaired = _run(monkeypatch, L, 0)
    paired = _run(monkeypatch, L, 1)
    for name, u, q in zip(FWD_OUT, unpaired, paired):
        assert bool(torch.isfinite(u).all()), name
        assert torch.equal(_bits(u), _bits(q)), (name, int((_bits(u) != _bits(q)).sum()))
    for t in paired:
        for b in (7, 18):
            assert torch.equal(_bits(t[b]), _bits(t[0])) and torch.equal(_bits(t[b + n]), _bits(t[n]))
    assert _same(paired, _run(monkeypatch, L, 1))


# ------------------------------------------------------------------ paired against float64: the two existing rules
@pytest.mark.parametrize("family", ["plain", "lowvar"])
@pytest.mark.parametrize("C,H,W,n", [(32, 5, 17, 1), (64, 5, 17, 3), (128, 5, 17, 1), (32, 19, 213, 19)])
def test_paired_vs_float64(monkeypatch, C, H, W, n, family):
    dev = _gpu()
    if (H, W, n) == WALK:
        _need_many_tiles_per_workgroup(dev)
    L, (s0, s1, p, m0, m1) = _twin_launch(dev, C, n, H, W, family=family)
    k = _fwd_refs(s0, s1, p, m0, m1, 2 * n)
    got = _run(monkeypatch, L, 1)
    _check_fwd("fwd-pair C=%d %dx%d n=%d %s" % (C, H, W, n, family), got, k, family)


# ------------------------------------------------------------------ a NaN stays in the pixels that read it
@pytest.mark.parametrize("where", ["interior", "bottom_right"])
@pytest.mark.parametrize("C", [32, 128])
def test_paired_nan_confinement(monkeypatch, C, where):
    dev = _gpu()
    n, H, W = 3, 5, 17
    y, x = (2, 7) if where == "interior" else (H - 1, W - 1)
    clean = _run(monkeypatch, _twin_launch(dev, C, n, H, W)[0], 1)

    def check(bad, hit):
        for name, c, d in zip(FWD_OUT, clean, bad):
            same = _bits(c) == _bits(d)
            for bb in hit:
                assert not bool(torch.isfinite(d[bb, y, x]).any()), (name, bb)     # the value really was read
                same[bb, y, x] = True
            assert bool(same.all()), name

    # a pixel of xs[1]: launch batches 1 and 1 + n read it (the shared half of z), nobody else
    def in_xs(s0, s1):
        s0[1, y, x, C // 2 + 1] = float("nan")
    check(_run(monkeypatch, _twin_launch(dev, C, n, H, W, edit=in_xs)[0], 1), (1, 1 + n))
    # a pixel of x12[j]: only launch batch (j + n) % 2n reads it -- the first half of pair 1 (j = 1 + n), the second (j = 1)
    for j in (1 + n, 1):
        def in_x12(s0, s1, j=j):
            s1[j, y, x, C // 2 + 1] = float("nan")
        check(_run(monkeypatch, _twin_launch(dev, C, n, H, W, edit=in_x12)[0], 1), ((j + n) % (2 * n),))


# ------------------------------------------------------------------ the switch
def _guarded(L):
    B, H, W, C = L.shape
    px = B * H * W
    outs = [Guarded(px * C, L.dev), Guarded(px, L.dev), Guarded(px * C, L.dev)]
    L.a.yhat, L.a.rstd, L.a.centre = (o.ptr() for o in outs)
    return outs


def _plain_launch(dev, C, B, H, W, nb0, m0):
    """A forward launch whose s0 is a tensor of nb0 images read through the batch map m0; s1 contiguous over B images."""
    s0, s1, p = R.fwd_inputs(C, nb0, B, H, W, "plain", 1234 + B)
    return FwdLaunch(dev, C, B, H, W, s0, s1, p, m0, (0, None), "contiguous")


@pytest.mark.parametrize("what,B,nb0,m0,reason", [
    ("odd B", 3, 3, (0, None), "odd"),
    ("s0 contiguous over 2n distinct images", 4, 4, (0, None), "different images"),
    ("s0 with mod = 2n", 4, 4, (0, 4), "different images"),
])
def test_forced_pair_refuses_unpairable_launches(monkeypatch, what, B, nb0, m0, reason):
    dev = _gpu()
    L = _plain_launch(dev, 32, B, 5, 17, nb0, m0)
    outs = _guarded(L)
    _mode(monkeypatch, 1)
    refused("_chain_fwd", "bmc_chain_fwd", ctypes.byref(L.a), match="bmc_chain_fwd.*" + SWITCH + ".*" + reason)
    assert all(o.untouched() for o in outs), what
    for mode in (0, None):                                                    # ... and launch unpaired otherwise
        _mode(monkeypatch, mode)
        outs = _guarded(L)
        call("_chain_fwd", "bmc_chain_fwd", ctypes.byref(L.a))
        assert not any(o.untouched() for o in outs), (what, mode)
        for o in outs:
            o.cpu()


@pytest.mark.parametrize("C", CS)
def test_switch_off_and_automatic_rule_on_pairable_launch(monkeypatch, C):
    """5 x 17 twin, n = 3: 12 pairs against 24 units, less than one per CU -- the rule keeps it unpaired.
    All three settings launch and agree in every bit."""
    dev = _gpu()
    L, _ = _twin_launch(dev, C, 3, 5, 17)
    off = _run(monkeypatch, L, 0)
    forced = _run(monkeypatch, L, 1)
    auto = _run(monkeypatch, L, None)
    assert all(bool(torch.isfinite(t).all()) for t in off)
    assert _same(off, forced) and _same(off, auto)


def test_automatic_rule_at_a_paired_shape(monkeypatch):
    """19 x 213, n = 19 at C = 32: 1330 pairs are 6 per CU on the fullest of 256 CUs, 2660 units 11 (30 < 33 steps): the rule
    pairs.  Whichever kernel the device's CU count selects, the bits are those of both forced forms."""
    dev = _gpu()
    H, W, n = WALK
    L, _ = _twin_launch(dev, 32, n, H, W)
    auto = _run(monkeypatch, L, None)
    assert _same(auto, _run(monkeypatch, L, 0)) and _same(auto, _run(monkeypatch, L, 1))
