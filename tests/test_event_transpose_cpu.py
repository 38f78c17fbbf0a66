"""Host side of the 8-way patch augmentation (event_dataset: "Transpose", bit 3 of a sample's flags), no GPU: the flag against
the random.Random draws written out by hand; plans that do not name it are what they were, call for call; crop_origin of a
transposed sample; the refusals; and the numpy statement of bmc_seq_encode_crop's contract for bit 3 that the GPU tests compare
the kernel with (tests/event_train_ref.encode_sample at the sample's full sizes with flips & 7, transposed, sliced)."""
import random

import numpy as np
import pytest
import torch

import event_train_ref as R
from test_event_crop_cpu import crop_slices

G, CASES = R.load_golden()
THREE = ("Horizontal", "Vertical", "Polarity")


def transposed_crop_slices(full_inp, full_gt, origin, crop, scale):
    """The contract of bmc_seq_encode_crop for a sample with bit 3 set: full frames [..., 2, H, W] / [..., 2, gh, gw] of
    flips & 7 -> the patches of the transposed frames at `origin`, which is in the transposed frames' rows / columns."""
    return crop_slices(full_inp.swapaxes(-1, -2), full_gt.swapaxes(-1, -2), origin, crop, scale)


def sample_slices(full_inp, full_gt, flips, origin, crop, scale):
    """A sample of either kind: the frames are those of flips & 7."""
    return (transposed_crop_slices if flips & 8 else crop_slices)(full_inp, full_gt, origin, crop, scale)


# ------------------------------------------------------------------ the flag
def _draw(seed):
    g = random.Random()
    g.seed(seed)
    return g.random()


@pytest.mark.parametrize("mechanisms", [THREE + ("Transpose",), ("Transpose",), ("Transpose", "Horizontal"),
                                        ("Vertical", "Rotate", "Transpose", "Polarity")])
def test_transpose_is_bit_3_from_one_draw_after_seed_plus_3(mechanisms):
    from bmc_hip.encodings import augment_flags
    from event_dataset import TRANSPOSE, sequence_plan
    assert TRANSPOSE == 8
    bits = {"Horizontal": 0, "Vertical": 1, "Polarity": 2, "Transpose": 3}
    probs = tuple(0.35 + 0.1 * i for i in range(len(mechanisms)))
    seen = set()
    for rs in range(40):
        rng = random.Random(rs)
        seed = random.Random(rs).randint(0, 2 ** 32)
        want = sum(1 << bits[m] for i, m in enumerate(mechanisms) if m in bits and _draw(seed + bits[m]) < probs[i])
        got_seed, items, paused, flips = sequence_plan(1, 20, 4, 2, (mechanisms, probs), None, rng)
        assert (got_seed, items, paused, flips) == (seed, [2, 3, 4, 5], [False] * 4, want)
        # the state afterwards: re-seeded for the last known mechanism, one draw taken
        last = [m for m in mechanisms if m in bits][-1]
        g = random.Random()
        g.seed(seed + bits[last])
        g.random()
        assert rng.getstate() == g.getstate()
        state = random.getstate()
        assert augment_flags(seed, mechanisms, probs) == want
        assert random.getstate() == g.getstate()                     # the module's generator: left re-seeded, as the reference
        random.setstate(state)
        seen.add(want & 8)
    assert seen == {0, 8}


def test_pause_chain_with_transpose_last_repeats_the_second_draw_after_seed_plus_3():
    from event_dataset import sequence_plan
    for rs in range(20):
        seed = random.Random(rs).randint(0, 2 ** 32)
        g = random.Random()
        g.seed(seed + 3)
        g.random()
        u = g.random()                                               # every pause draw of the sequence
        want, now = [False], False
        for _ in range(4):
            now = u < (0.6 if now else 0.3)
            want.append(now)
        assert sequence_plan(0, 30, 5, None, (THREE + ("Transpose",), (0.5,) * 4), (0.3, 0.6), random.Random(rs))[2] == want


def _plan_before(i, L, step, mechanisms, probs, pause, rng):
    """sequence_plan for the reference's three mechanisms, call for call, as it was before "Transpose" existed."""
    def flags():
        f = 0
        for k, mech in enumerate(mechanisms):
            bit = {"Horizontal": 0, "Vertical": 1, "Polarity": 2}.get(mech)
            if bit is None:
                continue
            rng.seed(seed + bit)
            if rng.random() < probs[k]:
                f |= 1 << bit
        return f
    seed = rng.randint(0, 2 ** 32)
    flips = flags()
    j, k, items, paused, now = i * step, 0, [i * step], [False], False
    for _ in range(L - 1):
        if pause is not None:
            now = rng.random() < (pause[1] if now else pause[0])
        k += 0 if now else 1
        items.append(j + k)
        paused.append(now)
        flags()
    return seed, items, paused, flips


@pytest.mark.parametrize("mechanisms", [THREE, ("Polarity", "Horizontal"), ("Vertical", "Rotate", "Horizontal")])
@pytest.mark.parametrize("pause", [None, (0.3, 0.6)])
def test_plans_that_do_not_name_transpose_are_unchanged_call_for_call(mechanisms, pause):
    from event_dataset import sequence_plan
    probs = (0.5, 0.4, 0.6)[:len(mechanisms)]
    for rs in range(30):
        a, b = random.Random(rs), random.Random(rs)
        got = sequence_plan(2, 40, 5, 3, (mechanisms, probs), pause, a)
        assert got == _plan_before(2, 5, 3, mechanisms, probs, pause, b)
        assert got[3] < 8 and a.getstate() == b.getstate()


def test_golden_plans_of_the_reference_are_unchanged():
    from event_dataset import sequence_plan
    for c in CASES.values():
        rng = random.Random(c["rs"])
        seed, items, paused, flips = sequence_plan(c["i"], len(G["lr_index"]), c["L"], c["step"], c["augment"], c["pause"], rng=rng)
        assert (seed, items, paused, flips) == (c["seed"], c["items"], c["paused"], c["flips"]) and flips < 8
        assert rng.random() == c["next"]


def test_probabilities_zero_and_one():
    from bmc_hip.encodings import augment_flags
    from event_dataset import sequence_plan
    state = random.getstate()
    for rs in range(25):
        for p, bit in ((0.0, 0), (1.0, 8)):
            flips = sequence_plan(0, 9, 3, None, (THREE + ("Transpose",), (0.5, 0.5, 0.5, p)), None, random.Random(rs))[3]
            assert flips & 8 == bit
            assert sequence_plan(0, 9, 3, None, (("Transpose",), (p,)), None, random.Random(rs))[3] == bit
            assert augment_flags(rs, ("Transpose",), (p,)) == bit
    random.setstate(state)


# ------------------------------------------------------------------ crop_origin
@pytest.mark.parametrize("lr_size,gt_size,crop,scale,max_top,max_left", [
    ((37, 53), (148, 212), (8, 12), 4, 45, 25),
    ((31, 56), (124, 222), (8, 12), 4, 47, 19),           # EventZoom: the ground truth is narrower than 4 x LR, so the
                                                          # transposed top is bounded by it: (222 - 32) // 4 = 47 < 56 - 8
    ((100, 120), (100, 120), (96, 96), 1, 24, 4),
    ((12, 53), (48, 212), (8, 12), 4, 45, 0),             # as wide as the transposed frame: left == 0 always
])
def test_crop_origin_of_a_transposed_sample_is_crop_origin_on_swapped_sizes(lr_size, gt_size, crop, scale, max_top, max_left):
    from event_dataset import crop_origin
    tops = set()
    for seed in list(range(60)) + [2 ** 32, 987654321]:
        g = random.Random(seed)
        want = (g.randint(0, max_top), g.randint(0, max_left))       # the same draws in the same order
        random.seed(5)
        before = random.getstate()
        got = crop_origin(seed, lr_size, gt_size, crop, scale, transpose=True)
        assert random.getstate() == before
        assert got == want == crop_origin(seed, lr_size[::-1], gt_size[::-1], crop, scale)
        assert crop_origin(seed, lr_size, gt_size, crop, scale, transpose=False) == crop_origin(seed, lr_size, gt_size, crop, scale)
        top, left = got
        assert top + crop[0] <= lr_size[1] and left + crop[1] <= lr_size[0]
        assert scale * (top + crop[0]) <= gt_size[1] and scale * (left + crop[1]) <= gt_size[0]
        tops.add(top)
    assert lr_size[0] - crop[0] < max(tops) <= max_top               # origins the frame as recorded could not hold


def test_crop_origin_refuses_a_patch_that_does_not_fit_the_transposed_frames():
    from event_dataset import crop_origin
    assert crop_origin(0, (12, 53), (48, 212), (8, 13), 4) is not None
    with pytest.raises(ValueError, match="does not fit"):
        crop_origin(0, (12, 53), (48, 212), (8, 13), 4, transpose=True)          # w = 13 > H = 12
    with pytest.raises(ValueError, match="does not fit"):
        crop_origin(0, (31, 56), (124, 222), (57, 12), 4)
    with pytest.raises(ValueError, match="does not fit"):
        crop_origin(0, (31, 56), (124, 222), (56, 12), 4, transpose=True)        # 4 * 56 > gw = 222


# ------------------------------------------------------------------ refusals
def _cols(side):
    return tuple(torch.tensor(G["%s_%s" % (side, c)]) for c in ("xs", "ys", "ps"))


def test_transpose_needs_crop_and_a_patch_that_fits_both_ways():
    from event_dataset import EventTrainSet
    aug = (THREE + ("Transpose",), (0.5,) * 4)
    with pytest.raises(ValueError, match='"Transpose" needs crop'):
        EventTrainSet(augment=aug)
    with pytest.raises(ValueError, match='"Transpose" needs crop'):
        EventTrainSet(augment=(("Transpose",), (0.0,)))
    assert EventTrainSet(augment=(THREE, (0.5,) * 3)).transposes is False
    ts = EventTrainSet(augment=aug, crop=(8, 12))
    assert ts.transposes and ts.last_flips is None and ts.last_origins is None

    H, W, gh, gw = G["size"].tolist()
    assert H != W and (gh, gw) == (4 * H, 4 * W)
    good = dict(lr=_cols("lr"), gt=_cols("gt"), lr_index=G["lr_index"], gt_index=G["gt_index"], lr_size=(H, W), gt_size=(gh, gw))
    one_way = (1, W) if W > H else (H, 1)                            # fits the frames as recorded, not transposed
    ts = EventTrainSet(L=4, augment=aug, crop=one_way)
    with pytest.raises(ValueError, match="does not fit the recording's .* transposed \\(\\(%d, %d\\) -> \\(%d, %d\\)\\)" % (W, H, gw, gh)):
        ts.add_recording(**good)
    assert len(ts) == 0
    # ... which a set that never transposes takes (the next refusal is the host columns'), as does this one a patch that fits both
    for ts in (EventTrainSet(L=4, augment=(THREE, (0.5,) * 3), crop=one_way), EventTrainSet(L=4, augment=aug, crop=(min(H, W),) * 2)):
        with pytest.raises(ValueError, match="GPU tensors"):
            ts.add_recording(**good)
    # the ground truth decides too: the transposed patch fits the LR frame and not an HR frame that is short of scale x LR
    crop, short = ((H - 1, H), (4 * H - 1, gw)) if W > H else ((W, W - 1), (gh, 4 * W - 1))
    with pytest.raises(ValueError, match="transposed"):
        EventTrainSet(L=4, augment=aug, crop=crop).add_recording(**dict(good, gt_size=short))
    with pytest.raises(ValueError, match="GPU tensors"):
        EventTrainSet(L=4, augment=(THREE, (0.5,) * 3), crop=crop).add_recording(**dict(good, gt_size=short))


def test_set_plans_carry_bit_3():
    from event_dataset import EventTrainSet
    ts = EventTrainSet(L=4, step_size=2, augment=(THREE + ("Transpose",), (0.5,) * 4), pause=(0.3, 0.6), crop=(8, 12))
    ts._recs.append(dict(lr_index=np.zeros((30, 2), np.int64), gt_index=np.zeros((30, 2), np.int64)))
    ts._ends.append((30 - 4) // 2 + 1)
    rng = random.Random(11)
    flips = [ts.plan(v, rng)[4] for v in range(len(ts))]
    assert {f & 8 for f in flips} == {0, 8} and max(flips) < 16


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", sorted(CASES))
def test_transposed_patch_is_the_transpose_of_the_swapped_patch(name):
    """The identity the contract implies, on the reference's own sequences: the transposed h x w patch at (top, left) is the
    transpose of the untransposed w x h patch at (left, top)."""
    from event_dataset import noise_events
    c = CASES[name]
    H, W, gh, gw = G["size"].tolist()
    noise = None if c["noise_level"] is None else noise_events(int(G["window"]), (H, W), c["seed"], c["noise_level"])
    lr, gt = (tuple(G["%s_%s" % (side, k)] for k in ("xs", "ys", "ps")) for side in ("lr", "gt"))
    full = R.encode_sample(lr, gt, G["lr_index"][c["items"]], G["gt_index"][c["items"]], c["flips"], c["paused"], (H, W), (gh, gw), noise)
    assert np.array_equal(full[0], c["inp"]) and np.array_equal(full[1], c["gt"])
    for (top, left), (h, w) in (((0, 0), (W, H)), ((W - 3, H - 2), (3, 2)), ((1, 2), (3, 2)), ((0, H - 2), (4, 2))):
        inp, out = transposed_crop_slices(*full, (top, left), (h, w), 4)
        assert inp.shape == c["inp"].shape[:2] + (h, w) and out.shape == c["gt"].shape[:2] + (4 * h, 4 * w)
        swapped = crop_slices(*full, (left, top), (w, h), 4)
        assert np.array_equal(inp, swapped[0].swapaxes(-1, -2)) and np.array_equal(out, swapped[1].swapaxes(-1, -2))
        # pixel for pixel: [r][c] of the transposed patch is [left + c][top + r] of the frame
        assert np.array_equal(inp[..., 1, 0], c["inp"][..., left, top + 1]) and np.array_equal(out[..., 2, 1], c["gt"][..., 4 * left + 1, 4 * top + 2])
        assert np.array_equal(sample_slices(*full, 8, (top, left), (h, w), 4)[1], out)
        assert np.array_equal(sample_slices(*full, 7, (left, top), (w, h), 4)[1], swapped[1])
    # the landing pixel of the out-of-range negatives, [gh-1][0] of channel 1, is [0][gh-1] of the transposed frame
    whole = transposed_crop_slices(*full, (0, 0), (W, H), 4)
    assert np.array_equal(whole[1][:, 1, 0, gh - 1], c["gt"][:, 1, gh - 1, 0])
