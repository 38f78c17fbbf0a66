"""The 8-way patch augmentation on the MI355X (bit 3 of bmc_seq_sample_t.flips, csrc/seq_encode.hip): bmc_seq_encode_crop against
the numpy statement of the contract (tests/test_event_transpose_cpu.transposed_crop_slices on tests/event_train_ref.encode_sample
at each sample's own full sizes with flips & 7), bit for bit: transposed and untransposed samples and two sensor sizes in one
launch, a ground truth smaller than scale x LR, the smallest shapes with more than one band, the (w, h)-at-(left, top) identity
on the GPU, full frames ignoring the bit, EventTrainSet.batch with "Transpose" against the transposed slices of full-frame
encodes of the same plans, bptt_step fed by it, the tool."""
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
from test_event_transpose_cpu import sample_slices
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_event_crop import N_ITEMS, _crop_sample, _guarded, _guards_intact, _set_recording, _tables
from test_gpu_event_train import _encode, _sample

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ helpers
def _encode_crops(dev, samples, L, crop, scale):
    """One bmc_seq_encode_crop launch into NaN-filled outputs between NaN guards -> (inp, gt) on the host."""
    from bmc_hip import encodings
    B, (h, w) = len(samples), crop
    table, crops, keep = _tables(dev, samples, L)
    bufs, outs = _guarded(dev, [(B, L, 2, h, w), (B, L, 2, scale * h, scale * w)])
    encodings.encode_sequence_crops(table, crops, B, L, crop, scale, out=tuple(outs))
    _guards_intact(bufs)
    return outs[0].cpu(), outs[1].cpu()


def _full(s):
    """The restatement's full frames of a sample: flips & 7 at its own sizes."""
    return R.encode_sample(s["lr"][0], s["gt"][0], s["lr_ranges"], s["gt_ranges"], s["flips"] & 7, s["paused"], s["size"], s["gsize"],
                           s["noise"])


def _want(samples, crop, scale):
    pairs = [sample_slices(*_full(s), s["flips"], s["origin"], crop, scale) for s in samples]
    return torch.from_numpy(np.stack([p[0] for p in pairs])), torch.from_numpy(np.stack([p[1] for p in pairs]))


def _check(dev, samples, L, crop, scale=4):
    inp, gt = _encode_crops(dev, samples, L, crop, scale)
    want_inp, want_gt = _want(samples, crop, scale)
    assert inp.dtype == gt.dtype == torch.float32
    assert inp.shape == want_inp.shape and gt.shape == want_gt.shape
    assert torch.equal(inp, want_inp) and torch.equal(gt, want_gt)
    assert not bool(torch.signbit(inp).any()) and not bool(torch.signbit(gt).any())          # zeros are +0.0
    return inp, gt


def _out_of_range_negatives(s):
    """Per range of the sample, LR then HR: the events that land on the quirk pixel -- negative after the polarity flip and
    outside the frame (a flip of a coordinate keeps an event on its side of the range test)."""
    sign = -1.0 if s["flips"] & 4 else 1.0
    counts = []
    for (xs, ys, ps), ranges, (fh, fw) in ((s["lr"][0], s["lr_ranges"], s["size"]), (s["gt"][0], s["gt_ranges"], s["gsize"])):
        for a, b in ranges:
            x, y, p = xs[a:b].astype(np.int64), ys[a:b].astype(np.int64), sign * ps[a:b]
            counts.append(int(((p < 0) & ((x < 0) | (x >= fw) | (y < 0) | (y >= fh))).sum()))
    return counts


# ------------------------------------------------------------------ 1. corners, interior, everything the table can say
def test_transposed_corners_interior_and_edges_beside_untransposed_samples_and_a_second_sensor():
    """37x53 -> 148x212, patch 8x12: the transposed frames are 53x37 -> 212x148, so origins run to (45, 25).  Eight transposed
    samples (flips 8..15) at the four corners, the interior and three edges, one with a paused item; two untransposed samples and
    two samples of a 31x56 -> 124x222 sensor in the same launch; noise with x == W and y == H in both polarities (_noise);
    out-of-range negatives in every range.  Their landing pixel, [fh-1][0] of channel 1, is [0][fh-1] of the transposed frame: in
    the patch at (0, 25) as column 36 - 25 = 11 (HR: 147 - 100 = 47), in no patch with top > 0."""
    dev = _gpu()
    size, gsize, crop, L = (37, 53), (148, 212), (8, 12), 3
    origins = [(0, 0), (0, 25), (45, 0), (45, 25), (20, 11), (45, 11), (7, 0), (0, 13)]
    rng = np.random.default_rng(12)
    samples = [_crop_sample(rng, dev, L, size, gsize, origins[b], 2048, 20000, flips=8 + b, paused=(1,) if b == 4 else (), a=3 + 2 * b)
               for b in range(8)]
    samples += [_crop_sample(rng, dev, L, size, gsize, o, 2048, 20000, flips=f, a=5) for o, f in (((29, 0), 3), ((13, 20), 6))]
    samples += [_crop_sample(rng, dev, L, (31, 56), (124, 222), o, 1500, 16000, flips=f, paused=(2,) if f & 8 else (), a=7)
                for o, f in (((40, 19), 13), ((23, 43), 5))]
    for s in samples:
        assert min(_out_of_range_negatives(s)) > 0
    inp, gt = _check(dev, samples, L, crop)
    # (0, 25) covers the landing pixel, LR and HR, in every item: events and noise
    assert bool((inp[1, :, 1, 0, 11] > 0).all()) and bool((gt[1, :, 1, 0, 47] > 0).all())
    full = _full(samples[1])
    assert np.array_equal(inp[1, :, 1, 0, 11].numpy(), full[0][:, 1, 36, 0]) and np.array_equal(gt[1, :, 1, 0, 47].numpy(), full[1][:, 1, 147, 0])
    # (45, 25) has the same columns and top > 0: the count is not there
    full = _full(samples[3])
    assert (full[1][:, 1, 147, 0] > gt[3, :, 1, 0, 47].numpy() + 5).all() and (full[0][:, 1, 36, 0] > inp[3, :, 1, 0, 11].numpy()).all()
    # ... and (0, 0) / (0, 13) have top == 0 and other columns
    for b in (0, 7):
        assert (_full(samples[b])[1][:, 1, 147, 0] > gt[b, :, 1, 0].numpy().max(-1) + 5).all()
    assert bool((inp[8, :, 1, -1, 0] > 0).all()) and bool((gt[8, :, 1, -1, 0] > 0).all())      # untransposed (29, 0): where it was
    assert not inp[4, 1].any() and gt[4, 1].any() and inp[4, 0].any()                            # the paused items
    assert not inp[10, 2].any() and gt[10, 2].any()
    assert len({inp[b].numpy().tobytes() for b in range(12)}) == 12
    # a transposed sample is not its untransposed patch (what a kernel that ignores bit 3 writes)
    plain = crop_slices(*_full(samples[4]), (20, 11), crop, 4)
    assert not np.array_equal(plain[1], gt[4].numpy())


# ------------------------------------------------------------------ 2. a ground truth smaller than scale x LR
def test_transposed_patch_at_the_largest_origin_of_a_narrow_ground_truth():
    """31x56 -> 124x222, transposed 56x31 -> 222x124: top <= min(56 - 8, (222 - 32) // 4) = 47, left <= min(31 - 12, 19) = 19."""
    dev = _gpu()
    import event_dataset as E
    assert E._max_origin((56, 31), (222, 124), (8, 12), 4) == (47, 19)
    rng = np.random.default_rng(13)
    samples = [_crop_sample(rng, dev, 3, (31, 56), (124, 222), (47, 19), 1500, 16000, flips=f, a=3 + 2 * b) for b, f in enumerate((8, 14))]
    inp, gt = _check(dev, samples, 3, (8, 12))
    assert gt[0, :, :, -4:].any() and gt[1, :, :, -4:].any()        # HR rows 216..219 of the transposed frame: sensor x up to 219


# ------------------------------------------------------------------ 3. more than one band
@pytest.mark.parametrize("size,gsize,crop,scale,t_origin,u_origin,n_lr,n_gt", [
    ((100, 120), (100, 120), (96, 96), 1, (0, 4), (4, 0), 9000, 9000),        # 9216 > 7680 counters: bands of 80 + 16 rows, LR and HR
    ((124, 130), (124, 130), (70, 120), 1, (0, 4), (54, 0), 9000, 9000),      # 15360 / 240 = 64: bands of 64 + 6 rows
    ((30, 40), (120, 160), (24, 24), 4, (0, 6), (6, 0), 2000, 20000),         # HR 96x96: 80 + 16; the LR patch is one band
])
def test_several_bands(size, gsize, crop, scale, t_origin, u_origin, n_lr, n_gt):
    """One transposed and one untransposed sample per launch.  The landing pixel of the out-of-range negatives is [0][fh-1] of
    the transposed sample's frame -- its first band -- and [fh-1][0] of the other's: its last."""
    dev = _gpu()
    h, w = crop
    assert 15360 // (2 * scale * w) < scale * h                      # the HR patch splits
    rng = np.random.default_rng(14)
    samples = [_crop_sample(rng, dev, 2, size, gsize, t_origin, n_lr, n_gt, flips=11, a=3),
               _crop_sample(rng, dev, 2, size, gsize, u_origin, n_lr, n_gt, flips=6, a=5)]
    for s in samples:
        assert min(_out_of_range_negatives(s)) > 0
    inp, gt = _check(dev, samples, 2, crop, scale)
    fh, gfh = size[0], gsize[0]
    assert t_origin[0] == 0 and u_origin[1] == 0 and u_origin[0] + h == fh
    assert bool((inp[0, :, 1, 0, fh - 1 - t_origin[1]] > 0).all()) and bool((gt[0, :, 1, 0, gfh - 1 - scale * t_origin[1]] > 3).all())
    assert bool((inp[1, :, 1, -1, 0] > 0).all()) and bool((gt[1, :, 1, -1, 0] > 3).all())
    rows = 15360 // (2 * scale * w)
    assert gt[0, :, :, rows:].any() and gt[1, :, :, rows:].any()    # the ragged last band holds events


# ------------------------------------------------------------------ 4. the identity, on the GPU
def test_transposed_launch_is_the_transpose_of_the_swapped_untransposed_launch():
    dev = _gpu()
    size, gsize, L = (37, 53), (148, 212), 3
    rng = np.random.default_rng(15)
    base = [_crop_sample(rng, dev, L, size, gsize, o, 2048, 20000, flips=f, paused=(2,) if b else (), a=3 + 2 * b)
            for b, (o, f) in enumerate((((45, 25), 5), ((20, 11), 2), ((0, 25), 7)))]
    transposed = [dict(s, flips=s["flips"] | 8) for s in base]
    swapped = [dict(s, origin=s["origin"][::-1]) for s in base]
    a = _encode_crops(dev, transposed, L, (8, 12), 4)
    b = _encode_crops(dev, swapped, L, (12, 8), 4)
    assert a[0].shape == (3, L, 2, 8, 12) and b[0].shape == (3, L, 2, 12, 8) and a[1].any()
    assert torch.equal(a[0], b[0].transpose(-1, -2)) and torch.equal(a[1], b[1].transpose(-1, -2))
    again = _encode_crops(dev, transposed, L, (8, 12), 4)
    assert again[0].numpy().tobytes() == a[0].numpy().tobytes() and again[1].numpy().tobytes() == a[1].numpy().tobytes()


# ------------------------------------------------------------------ 5. full frames ignore the bit
def test_full_frame_encoder_ignores_bit_3():
    dev = _gpu()
    size, gsize, L = (37, 53), (148, 212), 3
    rng = np.random.default_rng(16)
    base = [_crop_sample(rng, dev, L, size, gsize, (0, 0), 2048, 20000, flips=f, paused=(1,) if f == 5 else (), a=3 + f) for f in (0, 5, 7)]
    a = _encode(dev, base, L, size, gsize)
    b = _encode(dev, [dict(s, flips=s["flips"] | 8) for s in base], L, size, gsize)
    assert a[0].numpy().tobytes() == b[0].numpy().tobytes() and a[1].numpy().tobytes() == b[1].numpy().tobytes() and a[0].any()


# ------------------------------------------------------------------ 6. EventTrainSet.batch
FOUR = ("Horizontal", "Vertical", "Polarity", "Transpose")


def _kw(p):
    return dict(L=3, step_size=2, augment=(FOUR, (0.5, 0.5, 0.5, p)), pause=(0.4, 0.5), add_noise=0.1, window=128)


def _full_frames_of_plan(dev, ts, plan):
    """bmc_seq_encode's frames of one plan of the set with flips & 7 -> (inp [L,2,H,W], gt [L,2,gh,gw]) on the host."""
    import event_dataset as E
    r, seed, items, paused, flips = plan
    rec = ts._recs[r]
    H, W, gh, gw = rec["size"]
    s = _sample((None, rec["cols"][:3]), (None, rec["cols"][3:]), rec["lr_index"][items], rec["gt_index"][items], flips=flips & 7,
                paused=[t for t, p in enumerate(paused) if p], noise=E.noise_events(ts.window, (H, W), seed, ts.noise_level))
    inp, gt = _encode(dev, [s], ts.L, (H, W), (gh, gw))
    return inp[0], gt[0]


def _batch_against_full_frames(dev, ts, indices, rng, origins=None):
    import event_dataset as E
    c = random.Random()
    c.setstate(rng.getstate())
    plans = [ts.plan(v, c) for v in indices]                         # from a copy of the generator
    before = E.ENCODE_LAUNCHES
    inp, gt = ts.batch(indices, rng=rng, origins=origins)
    assert E.ENCODE_LAUNCHES == before + 1                           # one launch, whatever the mix
    assert rng.getstate() == c.getstate()
    B, (h, w), s = len(indices), ts.crop, ts.scale
    assert inp.shape == (B, ts.L, 2, h, w) and gt.shape == (B, ts.L, 2, s * h, s * w) and inp.is_contiguous() and gt.is_contiguous()
    assert ts.last_flips.dtype == np.int64 and ts.last_flips.tolist() == [p[4] for p in plans]
    assert ts.last_origins.dtype == np.int64 and ts.last_origins.shape == (B, 2)
    inp, gt = inp.cpu(), gt.cpu()
    for k, plan in enumerate(plans):
        H, W, gh, gw = ts._recs[plan[0]]["size"]
        tr = bool(plan[4] & 8)
        top, left = ts.last_origins[k].tolist()
        if origins is None:
            assert (top, left) == E.crop_origin(plan[1], (H, W), (gh, gw), ts.crop, s, transpose=tr)
        fi, fg = _full_frames_of_plan(dev, ts, plan)
        if tr:                                                       # in the output's own, transposed coordinates
            fi, fg = fi.transpose(-1, -2), fg.transpose(-1, -2)
        want_inp, want_gt = crop_slices(fi, fg, (top, left), ts.crop, s)
        assert want_inp.shape == inp[k].shape and want_gt.shape == gt[k].shape
        assert torch.equal(inp[k], want_inp) and torch.equal(gt[k], want_gt)
    assert gt.any() and not bool(torch.signbit(inp).any()) and not bool(torch.signbit(gt).any())
    return plans


@pytest.mark.parametrize("p", [1.0, 0.0, 0.5])
def test_batches_with_transpose_are_the_transposed_slices_of_the_full_frames_of_their_plans(p):
    dev = _gpu()
    import event_dataset as E
    ts = E.EventTrainSet(crop=(8, 12), scale=4, **_kw(p))
    for k in range(3):                                               # three sensor sizes share the set
        ts.add_recording(**_set_recording(dev, k))
    per = (N_ITEMS - 3) // 2 + 1
    assert len(ts) == 3 * per and ts.last_flips is None
    rng = random.Random(31)
    mixed = []
    for indices in ([per + 2, 1, 2 * per + 3, per, 4, 2 * per], [0, per + 1, 2 * per + 1, 3]):
        plans = _batch_against_full_frames(dev, ts, indices, rng)
        assert [q[0] for q in plans] == [v // per for v in indices]
        mixed.append({q[4] & 8 for q in plans})
    assert mixed == {1.0: [{8}, {8}], 0.0: [{0}, {0}], 0.5: [{0, 8}, {0, 8}]}[p]                 # at 0.5 both batches are mixed


def test_given_origins_are_checked_against_the_orientation_the_plan_drew():
    dev = _gpu()
    import event_dataset as E
    ts = E.EventTrainSet(crop=(8, 12), scale=4, **_kw(0.5))
    ts.add_recording(**_set_recording(dev, 0))                       # 37x53: origins to (29, 41) as recorded, (45, 25) transposed
    indices = [1, 4, 0, 5, 2, 3]

    def drawn(rng):
        c = random.Random()
        c.setstate(rng.getstate())
        return [bool(ts.plan(v, c)[4] & 8) for v in indices]

    corners = lambda tr: np.asarray([(45, 25) if t else (29, 41) for t in tr])
    rng = random.Random(31)
    tr = drawn(rng)
    assert True in tr and False in tr
    _batch_against_full_frames(dev, ts, indices, rng, origins=corners(tr))       # every sample at its own largest origin
    assert np.array_equal(ts.last_origins, corners(tr))
    state, tr = rng.getstate(), drawn(rng)
    assert True in tr and False in tr
    for k, t in enumerate(tr):                                       # ... and each refuses the other orientation's
        bad = corners(tr)
        bad[k] = (29, 41) if t else (45, 25)
        with pytest.raises(ValueError, match="origin \\(%d, %d\\) of sequence %d .*, %stransposed"
                           % (tuple(bad[k]) + (indices[k], "" if t else "not "))):
            ts.batch(indices, rng=rng, origins=bad)
        assert rng.getstate() == state                               # a refused batch has drawn nothing


# ------------------------------------------------------------------ 7. it feeds bptt_step
def test_a_bptt_step_on_a_transposed_batch():
    dev = _gpu()
    import event_dataset as E
    from test_gpu_multistream import _model
    from train_step import bptt_step
    ts = E.EventTrainSet(crop=(8, 12), scale=4, **_kw(1.0))
    ts.add_recording(**_set_recording(dev, 0))
    inp, gt = ts.batch([1, 4], rng=random.Random(21))
    assert ts.last_flips.tolist()[0] & 8 and ts.last_flips.tolist()[1] & 8
    m = _model(False, 16, n_b=1, seed=3, gain=1.5).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    loss, _ = bptt_step(m, opt, inp, gt, 16, 4)
    assert np.isfinite(loss.item()) and loss.item() > 0
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and any(bool(g.any()) for g in grads)


# ------------------------------------------------------------------ 8. the tool
def test_train_events_tool_trains_on_transposed_patches():
    _gpu()
    tool = os.path.join(ROOT, "tools", "train_events.py")
    p = subprocess.run([sys.executable, tool, "--synthetic", "3", "--size", "16x24,20x28", "--crop", "8x12", "--transpose", "--steps", "2",
                        "--L", "4", "--window", "128", "--sliding", "64", "--n-c", "16", "--n-b", "1"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    losses = [float(v) for v in re.findall(r"^step \d+  loss (\S+)  encode \S+ ms", p.stdout, re.M)]
    assert len(losses) == 2 and all(np.isfinite(losses)), p.stdout
    assert "8x12 patches, transposed with probability 0.5" in p.stdout
    p = subprocess.run([sys.executable, tool, "--synthetic", "3", "--transpose", "--steps", "2"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 2 and "--transpose needs --crop" in p.stdout, p.stdout
