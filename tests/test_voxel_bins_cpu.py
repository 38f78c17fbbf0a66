"""CPU tests of the voxel encoders' oracle at the bin counts and weights where rounding shows (tests/golden/voxel_bins.npz,
recorded from the reference by tests/golden/make_golden_voxel_bins.py):

* oracle.bmc_oracle.events_to_voxel_np / events_to_voxel_torch_np return every fixture's bytes, and the mutated coordinates;
* the fixtures discriminate: a restatement that fuses either of the encoders' two multiply-adds (tests/voxel_fused_ref.py)
  returns other bytes on them, so tests/test_gpu_voxel_bins.py cannot pass on a kernel that rounds in other places than the
  reference does.  The fused restatement is never an expected value."""
import os

import numpy as np
import pytest

import voxel_fused_ref as VF
from oracle import bmc_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))

MIN_DIFF = 8            # output elements in which a fused variant must differ from the fixture


def _load():
    z = np.load(os.path.join(HERE, "golden", "voxel_bins.npz"))
    out = {}
    for tag in z["cases"]:
        tag = str(tag)
        c = {k: z["%s/%s" % (tag, k)] for k in ("meta", "xs", "ys", "ts", "ps", "vox", "xs_after", "ys_after")}
        c["H"], c["W"], c["bins"] = (int(v) for v in c["meta"])
        out[tag] = c
    return out


CASES = _load()
V_TAGS = [t for t in CASES if t.startswith("v_")]
T_TAGS = [t for t in CASES if t.startswith("t_")]
EARLY_OUT = ("t_zero_ts", "t_three")


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def inexact_product(c):
    """bins - 1 is no power of two: t * (bins - 1) is rounded, so fusing it into the subtraction changes the result."""
    m = c["bins"] - 1
    return m & (m - 1) != 0


def float_weights(c):
    return bool((np.abs(c["ps"]) != 1).any())


def fused(tag, fuse):
    c = CASES[tag]
    fn = VF.voxel_torch if tag.startswith("t_") else VF.voxel
    return fn(c["xs"], c["ys"], c["ts"], c["ps"], c["bins"], c["H"], c["W"], fuse)


def ndiff(tag, fuse):
    return int((bits(fused(tag, fuse)) != bits(CASES[tag]["vox"])).sum())


def test_fixture_covers_the_listed_cases():
    for pre in ("v_", "t_"):
        pm = {CASES[t]["bins"] for t in CASES if t.startswith(pre + "pm")}
        fw = {CASES[t]["bins"] for t in CASES if t.startswith(pre + "fw")}
        assert pm == {4, 6, 7, 8, 10, 11, 33} and fw == {2, 5, 4, 7}
        assert all(not float_weights(CASES[t]) for t in CASES if t.startswith(pre + "pm"))
        assert all(float_weights(CASES[t]) for t in CASES if t.startswith(pre + "fw"))
        for name in ("wide6", "centres", "alloob", "1x1"):
            assert pre + name in CASES
    for tag, c in CASES.items():
        assert c["H"] <= 9 and c["W"] <= 11 and len(c["xs"]) <= 600, tag
        assert c["vox"].shape == (c["bins"], c["H"], c["W"]) and c["vox"].dtype == np.float32, tag
    c = CASES["v_centres"]
    k = c["ts"].astype(np.float64) * (c["bins"] - 1)
    assert np.array_equal(c["ts"], (np.round(k) / (c["bins"] - 1)).astype(np.float32)) and len(np.unique(c["ts"])) == c["bins"]
    c = CASES["v_outside"]
    assert c["ts"].min() < -0.1 and c["ts"].max() > 1.1
    for tag in ("v_alloob", "t_alloob"):
        c = CASES[tag]
        assert ((c["xs"] >= c["W"]) | (c["xs"] < 0) | (c["ys"] >= c["H"]) | (c["ys"] < 0)).all()
        assert not c["xs_after"].any() and not c["ys_after"].any() and not c["vox"][0].any() and c["vox"][1:].any()
    assert CASES["v_1x1"]["meta"][:2].tolist() == [1, 1] and CASES["t_1x1"]["meta"][:2].tolist() == [1, 1]
    for tag in T_TAGS:
        c = CASES[tag]
        assert np.array_equal(c["xs"], np.floor(c["xs"])) and np.array_equal(c["ys"], np.floor(c["ys"])), tag
    assert CASES["t_pm7"]["ts"].min() > 1.0 and CASES["t_norm"]["ts"][0] == 0 and CASES["t_norm"]["ts"].max() <= 1
    for tag in EARLY_OUT:                        # at a bin count that is no power of two plus one; nothing is touched
        c = CASES[tag]
        assert inexact_product(c) and not c["vox"].any()
        assert np.array_equal(c["xs_after"], c["xs"]) and np.array_equal(c["ys_after"], c["ys"])
    assert not CASES["t_zero_ts"]["ts"].any() and len(CASES["t_three"]["ts"]) == 3
    assert os.path.getsize(os.path.join(HERE, "golden", "voxel_bins.npz")) < 200 * 1024


@pytest.mark.parametrize("tag", V_TAGS)
def test_oracle_events_to_voxel_returns_the_reference_bytes(tag):
    c = CASES[tag]
    xs, ys = c["xs"].copy(), c["ys"].copy()
    vox, xa, ya = O.events_to_voxel_np(xs, ys, c["ts"], c["ps"], c["bins"], (c["H"], c["W"]))
    assert vox.dtype == np.float32 and np.array_equal(bits(vox), bits(c["vox"]))
    assert np.array_equal(bits(xa), bits(c["xs_after"])) and np.array_equal(bits(ya), bits(c["ys_after"]))
    assert np.array_equal(xs, c["xs"]) and np.array_equal(ys, c["ys"])          # (this oracle returns copies)


@pytest.mark.parametrize("tag", T_TAGS)
def test_oracle_events_to_voxel_torch_returns_the_reference_bytes(tag):
    c = CASES[tag]
    xs, ys, ps = c["xs"].copy(), c["ys"].copy(), c["ps"].copy()
    vox = O.events_to_voxel_torch_np(xs, ys, c["ts"], ps, c["bins"], (c["H"], c["W"]))
    assert vox.dtype == np.float32 and np.array_equal(bits(vox), bits(c["vox"]))
    assert np.array_equal(bits(xs), bits(c["xs_after"])) and np.array_equal(bits(ys), bits(c["ys_after"]))
    assert np.array_equal(bits(ps), bits(c["ps"]))                              # the weights it zeroes are temporaries


@pytest.mark.parametrize("tag", V_TAGS + T_TAGS)
def test_unfused_restatement_is_the_reference(tag):
    """The helper with no site fused returns the fixture: what the fused variants change is the fusion and nothing else."""
    assert np.array_equal(bits(fused(tag, None)), bits(CASES[tag]["vox"]))


@pytest.mark.parametrize("tag", [t for t in V_TAGS + T_TAGS if inexact_product(CASES[t]) and t not in EARLY_OUT])
def test_condition_a_fused_time_product_shows(tag):
    n = ndiff(tag, "t")
    print("%s: fusing t * (bins - 1) - b changes %d of %d elements" % (tag, n, CASES[tag]["vox"].size))
    assert n >= MIN_DIFF


@pytest.mark.parametrize("tag", [t for t in V_TAGS + T_TAGS if float_weights(CASES[t]) and t not in EARLY_OUT])
def test_condition_b_fused_accumulation_shows(tag):
    n = ndiff(tag, "acc")
    print("%s: fusing acc + p * w changes %d of %d elements" % (tag, n, CASES[tag]["vox"].size))
    assert n >= MIN_DIFF


@pytest.mark.parametrize("pre", ["v_", "t_"])
def test_condition_c_each_site_is_isolated_somewhere(pre):
    """+-1 weights: p * w is exact, so fusing the accumulation changes nothing and a mismatch on such a case at an inexact bin
    count is the time product's.  bins - 1 in {1, 4}: t * (bins - 1) is exact, so a mismatch on such a float-weight case is
    the accumulation's."""
    only_t = [t for t in CASES if t.startswith(pre + "pm") and inexact_product(CASES[t])]
    only_acc = [t for t in CASES if t.startswith(pre + "fw") and CASES[t]["bins"] - 1 in (1, 4)]
    assert len(only_t) >= 4 and len(only_acc) == 2
    for tag in only_t:
        assert ndiff(tag, "acc") == 0 and ndiff(tag, "t") >= MIN_DIFF, tag
    for tag in only_acc:
        assert ndiff(tag, "t") == 0 and ndiff(tag, "acc") >= MIN_DIFF, tag
