"""Patch training on the MI355X (event_dataset.EventTrainSet(crop=...), csrc/seq_encode.hip): bmc_seq_encode_crop against the
slices of the numpy restatement at each sample's own full sizes (tests/event_train_ref.encode_sample, pinned to the reference by
tests/golden/event_train.npz), bit for bit, at the smallest shapes where the band scheme takes another path; samples of
different sensor sizes in one launch; EventTrainSet.batch with crop against the slices of the full-frame batch; bptt_step fed
by it; the tool."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import event_train_ref as R
from test_event_crop_cpu import crop_slices
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_event_slots import _columns, _dev
from test_gpu_event_train import GUARD, _noise, _sample

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ helpers
def _recording(rng, dev, n_lr, n_gt, size, gsize):
    lr, gt = _columns(rng, n_lr, *size), _columns(rng, n_gt, *gsize)
    return (lr, _dev(lr, dev)), (gt, _dev(gt, dev))


def _ranges(n, L, a):
    """L overlapping ranges with odd starts, inside n events."""
    return [(a + t * (n // (L + 1)), min(a + (t + 2) * (n // (L + 1)) - 5, n)) for t in range(L)]


def _crop_sample(rng, dev, L, size, gsize, origin, n_lr, n_gt, flips=0, paused=(), noise=12, a=3):
    """A sample of test_gpu_event_train._sample with a recording of its own, its full sizes and its patch origin."""
    lr, gt = _recording(rng, dev, n_lr, n_gt, size, gsize)
    s = _sample(lr, gt, _ranges(n_lr, L, a), _ranges(n_gt, L, a), flips=flips, paused=paused,
                noise=_noise(rng, noise, *size) if noise else None)
    return dict(s, size=tuple(size), gsize=tuple(gsize), origin=tuple(origin))


def _tables(dev, samples, L):
    """-> (sample table, crop table, the noise tensors to keep alive) on the device."""
    import event_dataset as E
    B = len(samples)
    tab, crops, keep = np.zeros(B, E.SEQ_SAMPLE_DTYPE), np.zeros(B, E.SEQ_CROP_DTYPE), []
    for b, s in enumerate(samples):
        for name, t in zip(E.SEQ_SAMPLE_DTYPE.names[:6], s["lr"][1] + s["gt"][1]):
            tab[name][b] = t.data_ptr()
        tab["lr_range"][b, :L] = s["lr_ranges"]
        tab["gt_range"][b, :L] = s["gt_ranges"]
        tab["flips"][b] = s["flips"]
        tab["paused"][b] = sum(1 << t for t, p in enumerate(s["paused"]) if p)
        if s["noise"] is not None:
            nz = tuple(torch.tensor(np.ascontiguousarray(c)).to(dev) for c in s["noise"])
            keep.append(nz)
            tab["noise_xs"][b], tab["noise_ys"][b], tab["noise_ps"][b] = (t.data_ptr() for t in nz)
            tab["n_noise"][b] = len(s["noise"][0])
        crops[b] = s["size"] + s["gsize"] + s["origin"]
    return torch.from_numpy(tab.view(np.uint8).copy()).to(dev), torch.from_numpy(crops.view(np.uint8).copy()).to(dev), keep


def _guarded(dev, shapes):
    """NaN-filled outputs between NaN guards of GUARD floats -> (buffers, views)."""
    bufs, outs = [], []
    for shape in shapes:
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
        bufs.append(buf)
        outs.append(buf[GUARD:GUARD + n].view(shape))
    return bufs, outs


def _guards_intact(bufs):
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), "a guard region was written"


def _encode_crops(dev, samples, L, crop, scale):
    from bmc_hip import encodings
    B, (h, w) = len(samples), crop
    table, crops, keep = _tables(dev, samples, L)
    bufs, outs = _guarded(dev, [(B, L, 2, h, w), (B, L, 2, scale * h, scale * w)])
    got = encodings.encode_sequence_crops(table, crops, B, L, crop, scale, out=tuple(outs))
    assert got[0].data_ptr() == outs[0].data_ptr() and got[1].data_ptr() == outs[1].data_ptr()
    _guards_intact(bufs)
    return outs[0].cpu(), outs[1].cpu()


def _want(samples, crop, scale):
    """The oracle: the restatement at every sample's own full sizes, sliced as the contract says."""
    pairs = []
    for s in samples:
        full = R.encode_sample(s["lr"][0], s["gt"][0], s["lr_ranges"], s["gt_ranges"], s["flips"], s["paused"], s["size"], s["gsize"],
                               s["noise"])
        pairs.append(crop_slices(*full, s["origin"], crop, scale))
    return torch.from_numpy(np.stack([p[0] for p in pairs])), torch.from_numpy(np.stack([p[1] for p in pairs]))


def _check(dev, samples, L, crop, scale=4):
    inp, gt = _encode_crops(dev, samples, L, crop, scale)
    want_inp, want_gt = _want(samples, crop, scale)
    assert inp.dtype == gt.dtype == torch.float32
    assert inp.shape == want_inp.shape and gt.shape == want_gt.shape
    assert torch.equal(inp, want_inp) and torch.equal(gt, want_gt)
    assert not bool(torch.signbit(inp).any()) and not bool(torch.signbit(gt).any())          # zeros are +0.0
    return inp, gt, want_inp, want_gt


# ------------------------------------------------------------------ 1. the patch is the frame: bmc_seq_encode's bytes
def test_whole_frame_patch_equals_seq_encode():
    dev = _gpu()
    from bmc_hip import encodings
    size, gsize, B, L = (5, 7), (20, 28), 3, 3
    rng = np.random.default_rng(1)
    samples = [_crop_sample(rng, dev, L, size, gsize, (0, 0), 300, 4800, flips=(3 * b + 5) % 8, paused=(1,) if b == 0 else (), a=3 + 2 * b)
               for b in range(B)]
    inp, gt, _, _ = _check(dev, samples, L, size)
    table, _, keep = _tables(dev, samples, L)
    bufs, outs = _guarded(dev, [(B, L, 2) + size, (B, L, 2) + gsize])
    encodings.encode_sequences(table, B, L, size, gsize, out=tuple(outs))
    _guards_intact(bufs)
    assert outs[0].cpu().numpy().tobytes() == inp.numpy().tobytes() and outs[1].cpu().numpy().tobytes() == gt.numpy().tobytes()
    assert gt[:, :, 1, -1, 0].min() > 0                              # the out-of-range quirk is in every HR frame


# ------------------------------------------------------------------ 2. corners and interior, everything the table can say
def test_corners_and_interior_with_flips_pause_noise_and_out_of_range_events():
    """37x53 -> 148x212, patch 8x12: the four corners (max origin (29, 41)), the interior, three edges; flips 0..7; noise with
    x == W and y == H in both polarities; a paused item; out-of-range negatives in every range (_columns).  The quirk pixel of
    the full frame, [fh-1][0] of channel 1, is in the patch at (29, 0) and nowhere else."""
    dev = _gpu()
    size, gsize, crop, L = (37, 53), (148, 212), (8, 12), 3
    origins = [(0, 0), (0, 41), (29, 0), (29, 41), (13, 20), (29, 20), (7, 0), (0, 13)]
    rng = np.random.default_rng(2)
    samples = [_crop_sample(rng, dev, L, size, gsize, origins[b], 2048, 20000, flips=b, paused=(1,) if b == 4 else (), a=3 + 2 * b)
               for b in range(8)]
    inp, gt, want_inp, want_gt = _check(dev, samples, L, crop)
    assert bool((gt[2, :, 1, -1, 0] > 0).all())                      # (29, 0): the HR patch ends at [147][0], in every item
    assert bool((inp[2, :, 1, -1, 0] > 0).all())                     # ... and the LR patch at [36][0]: events and noise
    assert torch.equal(gt[0, :, 1, -1, 0], want_gt[0, :, 1, -1, 0]) and torch.equal(inp[0, :, 1, -1, 0], want_inp[0, :, 1, -1, 0])
    full = R.encode_sample(samples[0]["lr"][0], samples[0]["gt"][0], samples[0]["lr_ranges"], samples[0]["gt_ranges"], 0,
                           samples[0]["paused"], size, gsize, samples[0]["noise"])
    assert (full[1][:, 1, -1, 0] > gt[0, :, 1, -1, 0].numpy() + 5).all()          # the quirk's count stayed at the frame's [147][0]
    assert not inp[4, 1].any() and gt[4, 1].any()                    # the paused item: no LR patch, its HR patch
    assert len({inp[b].numpy().tobytes() for b in range(8)}) == 8
    again = _encode_crops(dev, samples, L, crop, 4)
    assert again[0].numpy().tobytes() == inp.numpy().tobytes() and again[1].numpy().tobytes() == gt.numpy().tobytes()


# ------------------------------------------------------------------ 3. / 4. several bands, the widest patch
def test_several_bands_with_a_ragged_last_one():
    """20x520 -> 80x2080, patch 11x500: the HR patch 44x2000 is 15 bands of 3 rows, the last with 2; the LR patch one band."""
    dev = _gpu()
    size, gsize, L = (20, 520), (80, 2080), 2
    rng = np.random.default_rng(3)
    samples = [_crop_sample(rng, dev, L, size, gsize, o, 6000, 60000, flips=f, a=3 + 2 * b)
               for b, (o, f) in enumerate((((9, 20), 3), ((0, 0), 6)))]
    inp, gt, _, _ = _check(dev, samples, L, (11, 500))
    assert gt[0, :, :, -2:].any() and gt[1, :, :, -2:].any()        # the ragged band holds events
    assert gt[:, :, 1, -1, 0].max() < 5                              # neither patch holds [79][0]: (9, 20) starts at column 80


def test_widest_patch_one_row_per_band():
    """2x1920 -> 8x7680, patch 1x1920 at (1, 0): the HR patch is rows 4..7 of the frame, a band is one row, and the last band
    holds the quirk pixel."""
    dev = _gpu()
    rng = np.random.default_rng(4)
    samples = [_crop_sample(rng, dev, 2, (2, 1920), (8, 7680), (1, 0), 4000, 30000, flips=5)]
    inp, gt, _, _ = _check(dev, samples, 2, (1, 1920))
    assert bool((gt[0, :, 1, -1, 0] > 5).all()) and bool((inp[0, :, 1, -1, 0] > 0).all())


# ------------------------------------------------------------------ 5. mixed sensors in one launch; another scale
def test_three_sensor_sizes_in_one_launch():
    """31x56 -> 124x222 (the ground truth is narrower than 4 x LR: left <= 43), 37x53 -> 148x212 and 16x24 -> 64x96."""
    dev = _gpu()
    rng = np.random.default_rng(5)
    samples = [_crop_sample(rng, dev, 3, (31, 56), (124, 222), (23, 43), 1500, 16000, flips=1, paused=(2,)),
               _crop_sample(rng, dev, 3, (37, 53), (148, 212), (29, 0), 2048, 20000, flips=6, a=5),
               _crop_sample(rng, dev, 3, (16, 24), (64, 96), (8, 12), 600, 8000, flips=0, a=7)]
    inp, gt, _, _ = _check(dev, samples, 3, (8, 12))
    assert gt[0].any() and gt[1].any() and gt[2].any() and bool((gt[1, :, 1, -1, 0] > 0).all())


def test_scale_two():
    dev = _gpu()
    rng = np.random.default_rng(6)
    samples = [_crop_sample(rng, dev, 3, (12, 20), (24, 40), o, 600, 2400, flips=f, a=3 + 2 * b)
               for b, (o, f) in enumerate((((6, 10), 7), ((0, 3), 2), ((6, 0), 0)))]
    _check(dev, samples, 3, (6, 10), scale=2)


# ------------------------------------------------------------------ 6. the shortest and the longest sequence
@pytest.mark.parametrize("L", [2, 32])
def test_shortest_and_longest_sequence(L):
    dev = _gpu()
    rng = np.random.default_rng(L)
    samples = [_crop_sample(rng, dev, L, (5, 7), (20, 28), o, 40 * L + 100, 640 * L + 100, flips=6 - b, paused=(L - 1,) if b else (),
                            noise=9, a=1 + b) for b, o in enumerate(((2, 3), (0, 0)))]
    _check(dev, samples, L, (3, 4))


# ------------------------------------------------------------------ 7. refusals
def test_encode_sequence_crops_refusals():
    dev = _gpu()
    import event_dataset as E
    from bmc_hip import encodings, lib
    table = torch.zeros(2 * E.SEQ_SAMPLE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    crops = torch.zeros(2 * E.SEQ_CROP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="bmc_seq_encode_crop: HR patches wider than 7680"):
        encodings.encode_sequence_crops(table, crops, 2, 2, (1, 1921), 4)              # 2 * scale * w > ENC_LDS
    assert "bmc_seq_encode_crop" in lib.bmc_last_error().decode()
    with pytest.raises(RuntimeError, match="bmc_seq_encode_crop: HR patches wider than 7680"):
        encodings.encode_sequence_crops(table, crops, 2, 2, (1, 7681), 1)
    for L in (1, E.MAX_ITEMS + 1):
        with pytest.raises(RuntimeError, match="bmc_seq_encode_crop: bad arguments"):
            encodings.encode_sequence_crops(table, crops, 2, L, (4, 4), 4)
    with pytest.raises(ValueError, match="fewer than 3 entries"):
        encodings.encode_sequence_crops(table, crops, 3, 2, (4, 4), 4)
    with pytest.raises(ValueError, match="crop table holds fewer than 2 entries"):
        encodings.encode_sequence_crops(table, crops[:24], 2, 2, (4, 4), 4)
    with pytest.raises(ValueError, match="positive"):
        encodings.encode_sequence_crops(table, crops, 2, 2, (4, 4), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        encodings.encode_sequence_crops(table.cpu(), crops, 2, 2, (4, 4), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        encodings.encode_sequence_crops(table, crops.cpu(), 2, 2, (4, 4), 4)
    good = (torch.empty(2, 2, 2, 4, 4, device=dev), torch.empty(2, 2, 2, 16, 16, device=dev))
    for out in ((good[0], torch.empty(1, device=dev)), (good[0], torch.empty(2, 2, 2, 8, 8, device=dev)), (good[1], good[1]),
                (good[0].double(), good[1])):
        with pytest.raises(ValueError, match="out must be"):
            encodings.encode_sequence_crops(table, crops, 2, 2, (4, 4), 4, out=out)


# ------------------------------------------------------------------ 8. EventTrainSet(crop=...)
SIZES = ((37, 53, 148, 212), (31, 56, 124, 222), (16, 24, 64, 96))
N_ITEMS, PER_ITEM = 14, 96


def _set_recording(dev, k):
    """Recording k: columns at SIZES[k] and index tables of N_ITEMS overlapping items, by hand."""
    H, W, gh, gw = SIZES[k]
    rng = np.random.default_rng(40 + k)
    n_lr = PER_ITEM * (N_ITEMS + 1) + 7
    lr, gt = _columns(rng, n_lr, H, W), _columns(rng, 16 * n_lr, gh, gw)
    lr_index = np.asarray([(3 + PER_ITEM * t, 3 + PER_ITEM * (t + 2)) for t in range(N_ITEMS)], np.int64)
    return dict(lr=_dev(lr, dev), gt=_dev(gt, dev), lr_index=lr_index, gt_index=16 * lr_index, lr_size=(H, W), gt_size=(gh, gw))


KW = dict(L=3, step_size=2, augment=(("Horizontal", "Vertical", "Polarity"), (0.5, 0.5, 0.5)), pause=(0.4, 0.5), add_noise=0.1, window=128)


def test_cropping_set_equals_the_slices_of_the_full_frame_set():
    dev = _gpu()
    import event_dataset as E
    rec = _set_recording(dev, 0)
    full, patch = E.EventTrainSet(**KW), E.EventTrainSet(crop=(8, 12), scale=4, **KW)
    full.add_recording(**rec)
    patch.add_recording(**rec)
    assert len(full) == len(patch) == (N_ITEMS - 3) // 2 + 1 and patch.last_origins is None
    a, b = random.Random(5), random.Random(5)
    seen = set()
    for indices in ([1, 4, 0, 5], [2, 3]):
        before = E.ENCODE_LAUNCHES
        inp, gt = patch.batch(indices, rng=a)
        assert E.ENCODE_LAUNCHES == before + 1                       # two batches: two launches
        B = len(indices)
        assert inp.shape == (B, 3, 2, 8, 12) and gt.shape == (B, 3, 2, 32, 48) and inp.is_cuda and inp.is_contiguous()
        state = b.getstate()
        full_inp, full_gt = full.batch(indices, rng=b)
        assert a.getstate() == b.getstate()
        c = random.Random()
        c.setstate(state)
        seeds = [full.plan(v, c)[1] for v in indices]
        origins = patch.last_origins
        assert origins.dtype == np.int64 and origins.shape == (B, 2)
        assert origins.tolist() == [list(E.crop_origin(s, (37, 53), (148, 212), (8, 12), 4)) for s in seeds]
        for k, o in enumerate(origins.tolist()):
            want_inp, want_gt = crop_slices(full_inp[k], full_gt[k], o, (8, 12), 4)
            assert torch.equal(inp[k], want_inp) and torch.equal(gt[k], want_gt)
            seen.add(tuple(o))
        assert inp.any() and not bool(torch.signbit(inp).any()) and not bool(torch.signbit(gt).any())
    assert len(seen) > 3
    # origins= overrides the rule and draws the same plans
    given = np.asarray([[29, 41], [0, 0]])
    a, b = random.Random(9), random.Random(9)
    inp, gt = patch.batch([2, 5], rng=a, origins=given)
    full_inp, full_gt = full.batch([2, 5], rng=b)
    assert np.array_equal(patch.last_origins, given) and a.getstate() == b.getstate()
    for k, o in enumerate(given.tolist()):
        want_inp, want_gt = crop_slices(full_inp[k], full_gt[k], o, (8, 12), 4)
        assert torch.equal(inp[k], want_inp) and torch.equal(gt[k], want_gt)
    # ... and is checked against the sample's recording
    for bad in ([[30, 0], [0, 0]], [[0, 0], [0, 42]], [[-1, 0], [0, 0]], [[0, 0]], [[0.0, 0.0], [1.0, 1.0]]):
        state = a.getstate()
        with pytest.raises(ValueError, match="origin"):
            patch.batch([2, 5], rng=a, origins=np.asarray(bad))
        assert a.getstate() == state
    with pytest.raises(ValueError, match="origins needs a set with crop"):
        full.batch([2, 5], origins=given)


def test_mixed_sensor_sizes_share_a_batch_only_with_crop():
    dev = _gpu()
    import event_dataset as E
    recs = [_set_recording(dev, k) for k in range(3)]
    patch = E.EventTrainSet(crop=(8, 12), scale=4, **KW)
    singles = []
    for rec in recs:
        patch.add_recording(**rec)
        one = E.EventTrainSet(**KW)
        one.add_recording(**rec)
        singles.append(one)
    per = len(singles[0])
    indices = [per + 2, 1, 2 * per + 3, per]                          # recordings 1, 0, 2, 1
    assert [patch.locate(v)[0] for v in indices] == [1, 0, 2, 1]
    a = random.Random(3)
    before = E.ENCODE_LAUNCHES
    inp, gt = patch.batch(indices, rng=a)
    assert E.ENCODE_LAUNCHES == before + 1 and inp.shape == (4, 3, 2, 8, 12) and gt.shape == (4, 3, 2, 32, 48)
    b = random.Random(3)
    for k, v in enumerate(indices):                                  # sample k is the slice of its own recording's full frames
        r, i = patch.locate(v)
        full_inp, full_gt = singles[r].batch([i], rng=b)
        H, W, gh, gw = SIZES[r]
        top, left = patch.last_origins[k].tolist()
        assert 0 <= top <= min(H - 8, (gh - 32) // 4) and 0 <= left <= min(W - 12, (gw - 48) // 4)
        want_inp, want_gt = crop_slices(full_inp[0], full_gt[0], (top, left), (8, 12), 4)
        assert torch.equal(inp[k], want_inp) and torch.equal(gt[k], want_gt)
    assert a.getstate() == b.getstate()
    # the narrower ground truth bounds the origin: left = 44 fits the LR frame of recording 1, not its HR frame
    with pytest.raises(ValueError, match="origin \\(0, 44\\)"):
        patch.batch([per], origins=np.asarray([[0, 44]]))
    patch.batch([per], origins=np.asarray([[23, 43]]))
    # a recording smaller than the patch; a set without crop and a second size
    with pytest.raises(ValueError, match="the 8x12 patch .* does not fit the recording's \\(7, 53\\) -> \\(148, 212\\)"):
        patch.add_recording(**dict(recs[0], lr_size=(7, 53)))
    with pytest.raises(ValueError, match="sizes differ"):
        singles[0].add_recording(**recs[1])
    assert len(patch._recs) == 3 and len(singles[0]._recs) == 1


# ------------------------------------------------------------------ 9. it feeds bptt_step
def test_two_bptt_steps_from_patch_batches_equal_steps_from_sliced_full_frame_batches():
    """n_c = 16, n_b = 1, 37x53, patch 8x12, B = 2, L = 3: losses and parameters after two steps, bit for bit."""
    dev = _gpu()
    import event_dataset as E
    from test_gpu_multistream import _model
    from train_step import bptt_step
    rec = _set_recording(dev, 0)
    full, patch = E.EventTrainSet(**KW), E.EventTrainSet(crop=(8, 12), scale=4, **KW)
    full.add_recording(**rec)
    patch.add_recording(**rec)
    batches = [[1, 4], [5, 0]]

    def sliced(idx, rng):
        state = rng.getstate()
        full_inp, full_gt = full.batch(idx, rng=rng)
        c = random.Random()
        c.setstate(state)
        pairs = [crop_slices(full_inp[k], full_gt[k], E.crop_origin(full.plan(v, c)[1], (37, 53), (148, 212), (8, 12), 4), (8, 12), 4)
                 for k, v in enumerate(idx)]
        return torch.stack([p[0] for p in pairs]).contiguous(), torch.stack([p[1] for p in pairs]).contiguous()

    def run(feed):
        m = _model(False, 16, n_b=1, seed=3, gain=1.5).to(dev)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        rng = random.Random(21)
        losses = []
        for idx in batches:
            inp, gt = feed(idx, rng)
            loss, _ = bptt_step(m, opt, inp, gt, 16, 4)
            losses.append(loss.item())
        return losses, [p.detach().cpu() for p in m.parameters()]

    by_patches = run(lambda idx, rng: patch.batch(idx, rng=rng))
    by_slices = run(sliced)
    assert by_patches[0] == by_slices[0] and all(np.isfinite(by_patches[0])) and by_patches[0][0] != by_patches[0][1]
    assert all(torch.equal(a, b) for a, b in zip(by_patches[1], by_slices[1]))


# ------------------------------------------------------------------ 10. the tool
def test_train_events_tool_trains_on_patches_of_mixed_sensors():
    _gpu()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_events.py"), "--synthetic", "3", "--size", "16x24,20x28",
                        "--crop", "8x12", "--steps", "2", "--L", "4", "--window", "128", "--sliding", "64", "--n-c", "16", "--n-b", "1"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    losses = [float(v) for v in re.findall(r"^step \d+  loss (\S+)  encode \S+ ms", p.stdout, re.M)]
    assert len(losses) == 2 and all(np.isfinite(losses)), p.stdout
    assert "8x12 patches" in p.stdout
