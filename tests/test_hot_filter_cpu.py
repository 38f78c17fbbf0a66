"""Hot-pixel filter, the parts that need no GPU (include/bmc_hip.h, "hot-pixel filter"): the numpy restatement against the
reference's own outputs (tests/golden/hot_filter.npz), the integer cmin rule against the float32 expression, the host's
argument checks and the C layout of the hot table."""
import os

import numpy as np
import pytest

import hot_filter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hot_filter.npz")


def golden_cases():
    z = np.load(GOLDEN)
    for k in range(int(z["n"])):
        idx, max_px, min_obvs, max_rate = z["params_%d" % k]
        yield k, z["rate_%d" % k], int(idx), int(max_px), int(min_obvs), float(max_rate), z["mask_%d" % k], z["after_%d" % k]


def test_restatement_equals_the_reference_outputs():
    n = over = nan = neg = below = 0
    for k, rate, idx, max_px, min_obvs, max_rate, mask, after in golden_cases():
        m, a = R.get_hot_event_mask_np(rate, idx, max_px, min_obvs, max_rate)
        assert m.tobytes() == mask.tobytes() and a.tobytes() == after.tobytes(), k
        n += 1
        over += int(idx > min_obvs and 0 < max_px < (rate > np.float32(max_rate)).sum())
        nan += int(np.isnan(rate).any())
        neg += int(max_rate < 0)
        below += int(idx <= min_obvs)
    assert n >= 36 and over >= 5 and nan >= 2 and neg >= 5 and below >= 3      # the file holds the cases it is meant to hold
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_integer_form_equals_the_reference_outputs_on_count_images():
    """Every golden case whose rates are count / idx: the integer form gives the reference's mask."""
    seen = 0
    for k, rate, idx, max_px, min_obvs, max_rate, mask, after in golden_cases():
        c = np.rint(rate.astype(np.float64) * idx)
        if np.isnan(rate).any() or not np.array_equal((c.astype(np.float32) / np.float32(idx)), rate) or (c < 0).any():
            continue
        seen += 1
        assert np.array_equal(R.mask_from_counts_np(c.astype(np.int64), idx, max_px, min_obvs, max_rate), mask.astype(np.uint8)), k
    assert seen >= 30


@pytest.mark.parametrize("max_rate", [0.0, 0.25, 0.5, 0.8, 1.0])
def test_cmin_rule_for_every_idx(max_rate):
    from bmc_hip import slots
    for idx in range(1, 301):
        c = np.arange(idx + 1)
        above = c.astype(np.float32) / np.float32(idx) > np.float32(max_rate)
        want = int(np.argmax(above)) if above.any() else idx + 1
        assert np.array_equal(above, c >= want)                               # the float32 quotient is monotone in c
        assert slots.hot_cmin(idx, 0, max_rate) == want == R.cmin_np(idx, max_rate), idx
    assert slots.hot_cmin(5, 0, 0.8) == 5                                     # float32(4) / float32(5) > 0.8 is False
    assert slots.hot_cmin(5, 5, 0.1) == 0 and slots.hot_cmin(6, 5, 0.1) == 1  # idx <= min_obvs: the item masks nothing
    assert slots.hot_cmin(9, 0, -0.5) == 1                                    # max_rate < 0: the pixels with a count
    with pytest.raises(ValueError):
        slots.hot_cmin(1 << 23, 0, 0.5)


def test_hot_filter_argument_checks():
    import torch
    from infer import MultiStreamSR, evaluate_recordings  # noqa: F401
    m = torch.nn.Identity()
    ok = dict(max_px=3, min_obvs=1, max_rate=0.6)
    assert MultiStreamSR(m, 2, hot_filter=ok).hot_filter == (3, 1, 0.6)
    assert MultiStreamSR(m, 2).hot_filter is None and MultiStreamSR(m, 2, hot_filter=None).hot_filter is None
    for bad, name in ((dict(ok, max_px=-1), "max_px"), (dict(ok, max_px=1.5), "max_px"), (dict(ok, min_obvs=-2), "min_obvs"),
                      (dict(ok, min_obvs=True), "min_obvs"), (dict(ok, max_rate=float("nan")), "max_rate"),
                      (dict(ok, max_rate=float("inf")), "max_rate"), (dict(ok, max_rate="0.5"), "max_rate"),
                      (dict(ok, enabled=True), "enabled"), ({k: v for k, v in ok.items() if k != "min_obvs"}, "min_obvs")):
        with pytest.raises(ValueError, match=name):
            MultiStreamSR(m, 2, hot_filter=bad)
    with pytest.raises(ValueError, match="hot_filter"):
        MultiStreamSR(m, 2, hot_filter=[3, 1, 0.6])
    import inspect
    assert "hot_filter" in inspect.signature(evaluate_recordings).parameters


def test_slot_table_hot_part():
    from bmc_hip import slots
    with pytest.raises(ValueError, match="hot=True needs events=True"):
        slots.SlotTable(2, "cpu", hot=True)
    assert slots.HOT_KERNELS == 1 and slots.HOT_MAX_ITEMS == 1 << 23


def test_library_exports_the_hot_filter():
    from bmc_hip import lib
    for name in ("bmc_slot_hot_update", "bmc_slot_encode_filtered", "bmc_hot_pixel_mask"):
        assert name in lib.EXPORTS and lib.has_symbol(name)
    src = open(os.path.join(ROOT, "bmcnet-esr_amd", "csrc", "Makefile")).read()
    assert src.count("slot_hot.hip") == 1


def test_slot_hot_struct_layout_matches_header():
    import abi_ref
    from bmc_hip import slots
    fields = ["hot_pixels", "hot_mask", "first_item", "new_from", "active", "cmin"]
    structs = abi_ref.compiled_header()[0]
    size, compiled = structs["bmc_slot_hot_t"]
    dt = slots.SLOT_HOT_DTYPE
    assert [size] + [compiled[f][0] for f in fields] + [compiled["cmin"][1] // 4, structs["bmc_slot_events_t"][0], structs["bmc_slot_t"][0]] == \
        [dt.itemsize] + [dt.fields[f][1] for f in fields] + [slots.MAX_SEQN, slots.SLOT_EVENTS_DTYPE.itemsize, slots.SLOT_DTYPE.itemsize]
    assert dt.fields["cmin"][0].base == np.dtype("<i4")
    assert dt.itemsize == 64 and dt.fields["cmin"][0].shape == (slots.MAX_SEQN,)
    assert slots.SLOT_EVENTS_DTYPE.itemsize == 192 and slots.SLOT_DTYPE.itemsize == 40         # the existing layouts stay
    assert not np.zeros(1, dt)["active"][0]                                                    # all zero = the inactive form


def test_restatement_on_a_planted_recording():
    """The planted stream the GPU tests use does what they need: ties above max_px, windows before and after min_obvs, the
    (0, 0) pixel cleared by an out-of-range event, a p = 0 last writer, an empty item."""
    rng = np.random.default_rng(5)
    hot = [(0, 0), (2, 3), (4, 6), (1, 1), (3, 2)]
    lr, index = R.planted_recording(rng, (5, 7), 9, 6, hot, empty_item=4, zero_last=(6, 1))
    f = R.filter_recording_np(lr, index, (5, 7), 3, 2, 0.6)
    assert (f["hot"][:2] == 0).all() and f["hot"].max() == 3 and (f["masks"][2:] == 0).any()
    assert (f["counts"][4] == f["counts"][3]).all()                           # the empty item observes nothing
    assert f["counts"][6][2, 3] == f["counts"][5][2, 3]                       # p = 0 was the last writer on hot pixel 1
    assert f["counts"][1][0, 0] == 1 and f["counts"][0][0, 0] == 1            # odd items: an out-of-range event clears (0, 0)
    for j in range(9):
        gone = f["masks"][j][::-1] == 0
        assert (f["frames"][j][:, gone] == 0).all() and np.array_equal(f["frames"][j][:, ~gone], f["raw"][j][:, ~gone])
    assert not np.array_equal(f["frames"], f["raw"])
