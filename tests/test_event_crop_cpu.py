"""Host side of patch training (event_dataset.EventTrainSet(crop=...)), no GPU: crop_origin against the random.Random draws
written out by hand; the layout of bmc_seq_crop_t against a C compile of the header; the exports; the argument refusals that
need no GPU; the slicing oracle the GPU tests compare bmc_seq_encode_crop with (tests/event_train_ref.encode_sample at the
sample's full sizes, sliced) against the reference's own sequences of tests/golden/event_train.npz, as a whole-frame patch."""
import os
import random

import numpy as np
import pytest
import torch

import event_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, CASES = R.load_golden()


def crop_slices(full_inp, full_gt, origin, crop, scale):
    """The contract of bmc_seq_encode_crop: full frames [..., 2, H, W] / [..., 2, gh, gw] -> the patches at `origin`."""
    (top, left), (h, w) = origin, crop
    return (full_inp[..., top:top + h, left:left + w],
            full_gt[..., scale * top:scale * (top + h), scale * left:scale * (left + w)])


# ------------------------------------------------------------------ crop_origin
@pytest.mark.parametrize("lr_size,gt_size,crop,scale,max_top,max_left", [
    ((37, 53), (148, 212), (8, 12), 4, 29, 41),
    ((8, 53), (32, 212), (8, 12), 4, 0, 41),              # max_top == 0: the patch is as tall as the frame
    ((5, 7), (20, 28), (5, 7), 4, 0, 0),                  # the whole frame
    ((31, 56), (124, 222), (8, 12), 4, 23, 43),           # a ground truth narrower than 4 x LR: (222 - 48) // 4 = 43 < 56 - 12
    ((12, 20), (24, 40), (6, 10), 2, 6, 10),
    ((180, 240), (700, 960), (64, 64), 4, 111, 176),      # ... and a shorter one: (700 - 256) // 4 = 111 < 180 - 64
])
def test_crop_origin_is_the_two_draws_of_a_generator_of_its_own(lr_size, gt_size, crop, scale, max_top, max_left):
    from event_dataset import crop_origin
    tops, lefts = set(), set()
    for seed in list(range(60)) + [2 ** 32, 123456789]:
        g = random.Random(seed)
        top = g.randint(0, max_top)
        left = g.randint(0, max_left)
        random.seed(99)
        before = random.getstate()
        assert crop_origin(seed, lr_size, gt_size, crop, scale) == (top, left)
        assert random.getstate() == before                          # the module's generator is not touched
        assert top + crop[0] <= lr_size[0] and left + crop[1] <= lr_size[1]
        assert scale * (top + crop[0]) <= gt_size[0] and scale * (left + crop[1]) <= gt_size[1]
        tops.add(top)
        lefts.add(left)
    assert (max_top == 0) == (tops == {0}) and (max_left == 0) == (lefts == {0})
    assert max(tops) <= max_top and max(lefts) <= max_left


def test_crop_origin_refuses_a_patch_that_does_not_fit():
    from event_dataset import crop_origin
    for lr_size, gt_size in (((7, 53), (148, 212)), ((37, 11), (148, 212)), ((37, 53), (31, 212)), ((37, 53), (148, 47))):
        with pytest.raises(ValueError, match="does not fit"):
            crop_origin(0, lr_size, gt_size, (8, 12), 4)


def test_plans_do_not_depend_on_crop():
    """The origin comes from the plan's seed, not from the caller's generator: a cropping set and a full-frame set driven by
    equal generators plan the same items, flips and pauses, and leave the generators in the same state."""
    from event_dataset import EventTrainSet
    kw = dict(L=4, step_size=2, augment=(("Horizontal", "Vertical", "Polarity"), (0.5, 0.5, 0.5)), pause=(0.3, 0.6), add_noise=0.1,
              window=64)
    sets = [EventTrainSet(**kw), EventTrainSet(crop=(8, 12), scale=4, **kw)]
    for ts in sets:
        ts._recs.append(dict(lr_index=np.zeros((30, 2), np.int64), gt_index=np.zeros((30, 2), np.int64)))
        ts._ends.append((30 - 4) // 2 + 1)
    a, b = random.Random(5), random.Random(5)
    for v in (0, 7, 13, 3):
        assert sets[0].plan(v, a) == sets[1].plan(v, b)
    assert a.random() == b.random()


# ------------------------------------------------------------------ argument checks that need no GPU
def _cols(side):
    return tuple(torch.tensor(G["%s_%s" % (side, c)]) for c in ("xs", "ys", "ps"))


def test_crop_set_arguments():
    from event_dataset import EventTrainSet, MAX_WIDTH
    for bad in (5, (5,), (5, 7, 9), "ab"):
        with pytest.raises(ValueError, match="crop must be None or"):
            EventTrainSet(crop=bad)
    for crop, scale in (((0, 7), 4), ((5, -1), 4), ((5, 7), 0), ((1, MAX_WIDTH // 4 + 1), 4), ((1, MAX_WIDTH), 2)):
        with pytest.raises(ValueError, match="scale \\* w at most 7680"):
            EventTrainSet(crop=crop, scale=scale)
    assert EventTrainSet(crop=(1, MAX_WIDTH // 4), scale=4).crop == (1, 1920)
    assert EventTrainSet().crop is None and EventTrainSet().last_origins is None

    H, W, gh, gw = G["size"].tolist()
    good = dict(lr=_cols("lr"), gt=_cols("gt"), lr_index=G["lr_index"], gt_index=G["gt_index"], lr_size=(H, W), gt_size=(gh, gw))
    ts = EventTrainSet(L=4, crop=(H, W), scale=gh // H)
    # a recording the patch does not fit: the message names its sizes and the crop
    for sizes in (dict(lr_size=(H - 1, W)), dict(lr_size=(H, W - 1)), dict(gt_size=(gh - 1, gw)), dict(gt_size=(gh, gw - 1))):
        with pytest.raises(ValueError, match="the %dx%d patch .* does not fit the recording's " % (H, W)) as e:
            ts.add_recording(**dict(good, **sizes))
        assert str(tuple(sizes.values())[0]) in str(e.value)
    with pytest.raises(ValueError, match="sizes must be positive"):
        ts.add_recording(**dict(good, gt_size=(gh, 0)))
    # any size the patch fits passes the size checks, wider than a full frame may be too: the next refusal is the host columns'
    for sizes in (dict(), dict(lr_size=(H + 3, W + 40), gt_size=(gh + 1, gw + 9)), dict(lr_size=(H, 9000), gt_size=(gh, 36000))):
        with pytest.raises(ValueError, match="GPU tensors"):
            ts.add_recording(**dict(good, **sizes))
    assert len(ts) == 0
    # without crop every check stands as it was
    with pytest.raises(ValueError, match="at most 7680 wide"):
        EventTrainSet(L=4).add_recording(**dict(good, gt_size=(gh, 7681)))
    with pytest.raises(ValueError, match="origins needs a set with crop"):
        EventTrainSet(L=4).batch([0], origins=np.zeros((1, 2), np.int64))


# ------------------------------------------------------------------ C ABI
def test_library_exports_seq_encode_crop():
    import ctypes as C
    from bmc_hip import lib
    assert "bmc_seq_encode_crop" in lib.EXPORTS and lib.has_symbol("bmc_seq_encode_crop")
    assert lib._seq_encode_crop.argtypes == [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3


def test_seq_crop_struct_layout_matches_header():
    import abi_ref
    import event_dataset as E
    from bmc_hip import encodings
    fields = E.SEQ_CROP_DTYPE.names
    assert fields == ("H", "W", "gh", "gw", "top", "left")
    size, compiled = abi_ref.compiled_header()[0]["bmc_seq_crop_t"]
    dt = E.SEQ_CROP_DTYPE
    assert [size] + [compiled[f][0] for f in fields] == [dt.itemsize] + [dt.fields[f][1] for f in fields]
    assert dt.itemsize == encodings.SEQ_CROP_BYTES == 24 and all(dt.fields[f][0] == np.dtype("<i4") for f in fields)
    assert E.SEQ_SAMPLE_DTYPE.itemsize % 8 == 0 and dt.itemsize % 8 == 0     # the crop entries and the noise columns stay aligned


# ------------------------------------------------------------------ the slicing oracle
@pytest.mark.parametrize("name", sorted(CASES))
def test_whole_frame_patch_of_the_restatement_is_the_reference_sequence(name):
    from event_dataset import crop_origin, noise_events, sequence_plan
    c = CASES[name]
    seed, items, paused, flips = sequence_plan(c["i"], len(G["lr_index"]), c["L"], c["step"], c["augment"], c["pause"],
                                               rng=random.Random(c["rs"]))
    H, W, gh, gw = G["size"].tolist()
    assert (gh, gw) == (4 * H, 4 * W)
    noise = None if c["noise_level"] is None else noise_events(int(G["window"]), (H, W), seed, c["noise_level"])
    lr, gt = (tuple(G["%s_%s" % (side, k)] for k in ("xs", "ys", "ps")) for side in ("lr", "gt"))
    full = R.encode_sample(lr, gt, G["lr_index"][items], G["gt_index"][items], flips, paused, (H, W), (gh, gw), noise)
    origin = crop_origin(seed, (H, W), (gh, gw), (H, W), 4)
    assert origin == (0, 0)
    inp, out = crop_slices(*full, origin, (H, W), 4)
    assert np.array_equal(inp, c["inp"]) and np.array_equal(out, c["gt"])
    # ... and a smaller patch is the same pixels of it
    inp, out = crop_slices(*full, (2, 3), (4, 5), 4)
    assert np.array_equal(inp, c["inp"][:, :, 2:6, 3:8]) and np.array_equal(out, c["gt"][:, :, 8:24, 12:32])
