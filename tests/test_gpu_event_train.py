"""Training from raw event columns on the MI355X (event_dataset.EventTrainSet, csrc/seq_encode.hip): bmc_seq_encode against the
numpy restatement (tests/event_train_ref.py, pinned to the reference by tests/golden/event_train.npz) bit for bit, at the sizes
where the band scheme takes another path; EventTrainSet.batch against the reference's own sequences; bptt_step fed by it."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import event_train_ref as R
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_event_slots import _columns, _dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096                       # floats of NaN before and after each output


# ------------------------------------------------------------------ helpers
def _sample(lr, gt, lr_ranges, gt_ranges, flips=0, paused=(), noise=None):
    """lr, gt: (host columns, device columns); paused: the item numbers; noise: (xs int16, ys int16, ps int8) host columns."""
    return dict(lr=lr, gt=gt, lr_ranges=np.asarray(lr_ranges, np.int64), gt_ranges=np.asarray(gt_ranges, np.int64), flips=flips,
                paused=[t in paused for t in range(len(lr_ranges))], noise=noise)


def _encode(dev, samples, L, size, gsize):
    """The kernel on a table built by hand, into NaN-filled outputs between NaN guards -> (inp, gt) on the host."""
    import event_dataset as E
    from bmc_hip import encodings
    B = len(samples)
    tab = np.zeros(B, E.SEQ_SAMPLE_DTYPE)
    keep = []
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
    table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    bufs, outs = [], []
    for h, w in (size, gsize):
        n = B * L * 2 * h * w
        buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
        bufs.append(buf)
        outs.append(buf[GUARD:GUARD + n].view(B, L, 2, h, w))
    got = encodings.encode_sequences(table, B, L, size, gsize, out=tuple(outs))
    assert got[0].data_ptr() == outs[0].data_ptr() and got[1].data_ptr() == outs[1].data_ptr()
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), "a guard region was written"
    return outs[0].cpu(), outs[1].cpu()


def _want(samples, size, gsize):
    pairs = [R.encode_sample(s["lr"][0], s["gt"][0], s["lr_ranges"], s["gt_ranges"], s["flips"], s["paused"], size, gsize, s["noise"])
             for s in samples]
    return torch.from_numpy(np.stack([p[0] for p in pairs])), torch.from_numpy(np.stack([p[1] for p in pairs]))


def _check(dev, samples, L, size, gsize):
    inp, gt = _encode(dev, samples, L, size, gsize)
    want_inp, want_gt = _want(samples, size, gsize)
    assert inp.dtype == gt.dtype == torch.float32
    assert torch.equal(inp, want_inp) and torch.equal(gt, want_gt)
    assert not bool(torch.signbit(inp).any()) and not bool(torch.signbit(gt).any())          # zeros are +0.0
    return inp, gt


def _recording(rng, dev, n_lr, n_gt, size, gsize, hot=0):
    lr, gt = _columns(rng, n_lr, *size, hot=hot), _columns(rng, n_gt, *gsize, hot=hot)
    return (lr, _dev(lr, dev)), (gt, _dev(gt, dev))


def _noise(rng, n, H, W):
    """Noise columns as add_noise_event gives them, with x == W, y == H and both polarities in."""
    xs, ys = rng.integers(0, W, n).astype(np.int16), rng.integers(0, H, n).astype(np.int16)
    ps = (rng.integers(0, 2, n) * 2 - 1).astype(np.int8)
    xs[0], ps[0] = W, -1
    xs[1], ps[1] = W, 1
    ys[2], ps[2] = H, -1
    ys[3], ps[3] = H, 1
    ps[4], ps[5] = -1, 1
    return xs, ys, ps


# ------------------------------------------------------------------ 1. the kernel at the sizes where the band scheme changes
@pytest.mark.parametrize("H,W,gh,gw,B,L,n_lr,n_gt", [
    (5, 7, 20, 28, 3, 3, 300, 4800),              # one band each
    (37, 53, 148, 212, 2, 3, 2048, 20000),        # 5 HR bands of 36 rows, the last one ragged with 4
    (180, 240, 720, 960, 1, 2, 6000, 60000),      # 6 LR bands of 32 rows (the last 20), 90 HR bands of 8
    (2, 7680, 3, 7680, 1, 2, 4000, 6000),         # the widest frame: a band is one row
])
def test_seq_encode_sizes(H, W, gh, gw, B, L, n_lr, n_gt):
    dev = _gpu()
    rng = np.random.default_rng(7 + H)
    samples = []
    for b in range(B):
        lr, gt = _recording(rng, dev, n_lr, n_gt, (H, W), (gh, gw), hot=n_lr // 8)
        a = 3 + 2 * b
        # overlapping, odd starts; the ends stay inside the columns (the kernel trusts its ranges: with a = 7 the last one
        # would otherwise read two events past them, whatever the allocator left there, where numpy's slice stops)
        lr_r = [(a + t * (n_lr // (L + 1)), min(a + (t + 2) * (n_lr // (L + 1)) - 5, n_lr)) for t in range(L)]
        gt_r = [(a + t * (n_gt // (L + 1)), min(a + (t + 2) * (n_gt // (L + 1)) - 5, n_gt)) for t in range(L)]
        samples.append(_sample(lr, gt, lr_r, gt_r, flips=(3 * b + 5) % 8, paused=(1,) if b == 0 and L > 2 else (),
                               noise=_noise(rng, 40, H, W)))
    inp, gt = _check(dev, samples, L, (H, W), (gh, gw))
    assert gt[:, :, 1, gh - 1, 0].min() > 0                          # the out-of-range quirk is in every HR frame


# ------------------------------------------------------------------ 2. everything the table can say, at the smallest size
def test_seq_encode_flips_pause_noise_and_odd_ranges():
    """B = 8: every flip value; samples from two recordings; overlapping ranges, an empty range, a frame whose events are all out
    of range, polarity 0 events (in _columns); paused items at t = 0, in the middle and last; noise with x == W, y == H and both
    polarities, on some samples only; a second launch gives the same bytes."""
    dev = _gpu()
    H, W, gh, gw, L = 5, 7, 20, 28, 5
    rng = np.random.default_rng(11)
    recs = [_recording(rng, dev, 700, 9000, (H, W), (gh, gw), hot=50) for _ in range(2)]
    for lr, gt in recs:                                              # events 600..639 / 8000..8399: all out of range, both signs
        (xs, ys, ps), (gx, gy, gp) = lr[0], gt[0]
        xs[600:620], ys[620:640] = W + 1, -2
        gx[8000:8200], gy[8200:8400] = -1, gh
        ps[600:640] = np.where(np.arange(40) % 2, 1.0, -1.0)
        gp[8000:8400] = np.where(np.arange(400) % 3, 1.0, -1.0)
        ps[[60, 120]], gp[[100, 1500]] = 0.0, 0.0                    # polarity 0 inside every sample's first ranges
    recs = [((lr[0], _dev(lr[0], dev)), (gt[0], _dev(gt[0], dev))) for lr, gt in recs]
    samples = []
    for b in range(8):
        lr, gt = recs[b % 2]
        a = 7 * b + 1
        lr_r = [(a, a + 128), (a + 64, a + 192), (600, 640), (333, 333), (a + 100, a + 350)]
        gt_r = [(a, a + 2048), (a + 1000, a + 3048), (8000, 8400), (4444, 4444), (a + 5000, a + 7000)]
        paused = {2: (0,), 3: (2,), 4: (4,), 5: (0, 1, 2, 3, 4), 6: (1, 3)}.get(b, ())
        samples.append(_sample(lr, gt, lr_r, gt_r, flips=b, paused=paused, noise=_noise(rng, 12 + b, H, W) if b % 3 else None))
    inp, gt = _check(dev, samples, L, (H, W), (gh, gw))
    assert not inp[5].any() and gt[5].any()                          # all items paused: no LR frame, every HR frame
    assert not inp[0, 3].any() and not gt[0, 3].any()                # the empty ranges: all-zero frames, written
    assert inp[0, 2].sum() == inp[0, 2, 1, H - 1, 0] == 20           # all out of range: only the 20 negatives count, at [H-1][0]
    assert len({inp[b].numpy().tobytes() for b in range(8)}) == 8
    again = _encode(dev, samples, L, (H, W), (gh, gw))
    assert again[0].numpy().tobytes() == inp.numpy().tobytes() and again[1].numpy().tobytes() == gt.numpy().tobytes()


@pytest.mark.parametrize("L", [2, 32])
def test_seq_encode_shortest_and_longest_sequence(L):
    dev = _gpu()
    H, W, gh, gw = 6, 9, 24, 36
    rng = np.random.default_rng(L)
    samples = []
    for b in range(2):
        lr, gt = _recording(rng, dev, 40 * L + 100, 640 * L + 100, (H, W), (gh, gw))
        samples.append(_sample(lr, gt, [(40 * t + b, 40 * t + 90) for t in range(L)], [(640 * t + b, 640 * t + 700) for t in range(L)],
                               flips=6 - b, paused=(L - 1,) if b else (), noise=_noise(rng, 9, H, W)))
    _check(dev, samples, L, (H, W), (gh, gw))


def test_encode_sequences_refusals():
    dev = _gpu()
    import event_dataset as E
    from bmc_hip import encodings
    table = torch.zeros(2 * E.SEQ_SAMPLE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="bad arguments"):
        encodings.encode_sequences(table, 2, E.MAX_ITEMS + 1, (4, 4), (8, 8))
    with pytest.raises(RuntimeError, match="bad arguments"):
        encodings.encode_sequences(table, 2, 1, (4, 4), (8, 8))
    with pytest.raises(RuntimeError, match="wider than 7680"):
        encodings.encode_sequences(table, 2, 2, (4, 4), (1, 7681))
    with pytest.raises(ValueError, match="fewer than 3 entries"):
        encodings.encode_sequences(table, 3, 2, (4, 4), (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        encodings.encode_sequences(table.cpu(), 2, 2, (4, 4), (8, 8))
    with pytest.raises(ValueError, match="out must be"):
        encodings.encode_sequences(table, 2, 2, (4, 4), (8, 8), out=(torch.empty(2, 2, 2, 4, 4, device=dev), torch.empty(1, device=dev)))


# ------------------------------------------------------------------ 3. EventTrainSet
G, CASES = R.load_golden()
SIZE, GSIZE = tuple(G["size"].tolist()[:2]), tuple(G["size"].tolist()[2:])


def _golden_cols(side, dev):
    return tuple(torch.tensor(G["%s_%s" % (side, c)]).to(dev) for c in ("xs", "ys", "ps"))


def _golden_set(dev, c, recordings=1):
    from event_dataset import EventTrainSet
    ts = EventTrainSet(L=c["L"], step_size=c["step"], augment=c["augment"], pause=c["pause"], add_noise=c["noise_level"],
                       window=int(G["window"]))
    for _ in range(recordings):
        ts.add_recording(_golden_cols("lr", dev), _golden_cols("gt", dev), G["lr_index"], G["gt_index"], SIZE, GSIZE)
    return ts


@pytest.mark.parametrize("name", sorted(CASES))
def test_batch_matches_reference_sequence(name):
    """random.seed(rs); batch([i]) is the reference's dataset[i] after the same seeding, and leaves `random` where it does."""
    dev = _gpu()
    import event_dataset as E
    c = CASES[name]
    ts = _golden_set(dev, c)
    assert len(ts) == (len(G["lr_index"]) - c["L"]) // (c["step"] or c["L"]) + 1
    random.seed(c["rs"])
    before = E.ENCODE_LAUNCHES
    inp, gt = ts.batch([c["i"]])
    assert E.ENCODE_LAUNCHES == before + 1
    assert random.random() == c["next"]
    assert inp.shape == (1, c["L"], 2) + SIZE and gt.shape == (1, c["L"], 2) + GSIZE and inp.is_cuda and gt.is_cuda
    assert torch.equal(inp[0].cpu(), torch.from_numpy(c["inp"])) and torch.equal(gt[0].cpu(), torch.from_numpy(c["gt"]))


def _restated_batch(ts, indices, rng):
    """What batch(indices, rng) must return, from the plans and the numpy restatement."""
    from event_dataset import noise_events
    out = []
    for v in indices:
        r, seed, items, paused, flips = ts.plan(v, rng)
        noise = noise_events(ts.window, SIZE, seed, ts.noise_level) if ts.noise_level is not None else None
        lr, gt = tuple(G["lr_" + k] for k in ("xs", "ys", "ps")), tuple(G["gt_" + k] for k in ("xs", "ys", "ps"))
        out.append(R.encode_sample(lr, gt, G["lr_index"][items], G["gt_index"][items], flips, paused, SIZE, GSIZE, noise))
    return torch.from_numpy(np.stack([o[0] for o in out])), torch.from_numpy(np.stack([o[1] for o in out]))


def test_batches_of_several_sequences_one_launch_each_and_repeatable():
    """B = 3 from two recordings, augmentation + pause + noise: one launch per batch, the restatement's frames, the same bytes
    when called again with the same generator state; a larger batch after a smaller one (the table grows)."""
    dev = _gpu()
    import event_dataset as E
    c = CASES["pause_degenerate"]
    ts = _golden_set(dev, c, recordings=2)
    per = len(ts) // 2
    for indices in ([1, per + 2, per - 1], [0, 2 * per - 1, 3, per, 5]):
        assert {ts.locate(v)[0] for v in indices} == {0, 1}
        before = E.ENCODE_LAUNCHES
        inp, gt = ts.batch(indices, rng=random.Random(5))
        assert E.ENCODE_LAUNCHES == before + 1
        want_inp, want_gt = _restated_batch(ts, indices, random.Random(5))
        assert torch.equal(inp.cpu(), want_inp) and torch.equal(gt.cpu(), want_gt)
        inp2, gt2 = ts.batch(indices, rng=random.Random(5))
        assert E.ENCODE_LAUNCHES == before + 2 and inp2.data_ptr() != inp.data_ptr()
        assert inp2.cpu().numpy().tobytes() == inp.cpu().numpy().tobytes() and gt2.cpu().numpy().tobytes() == gt.cpu().numpy().tobytes()
    with pytest.raises(IndexError):
        ts.batch([len(ts)])
    with pytest.raises(ValueError, match="1 <= B"):
        ts.batch([])


def test_add_recording_refusals_on_the_gpu():
    dev = _gpu()
    from event_dataset import EventTrainSet
    ts = _golden_set(dev, CASES["plain"])
    lr, gt = _golden_cols("lr", dev), _golden_cols("gt", dev)
    good = dict(lr=lr, gt=gt, lr_index=G["lr_index"], gt_index=G["gt_index"], lr_size=SIZE, gt_size=GSIZE)
    with pytest.raises(ValueError, match="sizes differ"):
        ts.add_recording(**dict(good, lr_size=(SIZE[0] + 1, SIZE[1])))
    bad = lr[2].clone()
    bad[17] = 0.5
    with pytest.raises(ValueError, match="lr polarities must be -1, 0 or \\+1"):
        ts.add_recording(**dict(good, lr=(lr[0], lr[1], bad)))
    far = G["gt_index"].copy()
    far[-1, 1] = gt[0].numel() + 1
    with pytest.raises(ValueError, match="gt_index has a range outside"):
        ts.add_recording(**dict(good, gt_index=far))
    with pytest.raises(ValueError, match="L <= 32"):
        EventTrainSet(L=33)
    assert len(ts._recs) == 1
    assert ts.add_recording(**good) == 1 and len(ts) == 2 * ((len(G["lr_index"]) - 5) // 5 + 1)


# ------------------------------------------------------------------ 4. it feeds bptt_step
def test_two_bptt_steps_from_event_batches_equal_steps_from_restated_frames():
    """n_c = 16, n_b = 2, 9x16, B = 2, L = 4: loss and parameters after two steps, bit for bit."""
    dev = _gpu()
    from test_gpu_multistream import _model
    from train_step import bptt_step
    c = dict(CASES["flips_all"], L=4, step=3, pause=(0.3, 0.5))
    ts = _golden_set(dev, c)
    batches = [[1, 4], [6, 0]]

    def run(feed):
        m = _model(False, 16, n_b=2, seed=3, gain=1.5).to(dev)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        rng = random.Random(21)
        losses = []
        for idx in batches:
            inp, gt = feed(idx, rng)
            loss, _ = bptt_step(m, opt, inp, gt, 16, 4)
            losses.append(loss.item())
        return losses, [p.detach().cpu() for p in m.parameters()]

    by_events = run(lambda idx, rng: ts.batch(idx, rng=rng))
    by_frames = run(lambda idx, rng: tuple(t.to(dev) for t in _restated_batch(ts, idx, rng)))
    assert by_events[0] == by_frames[0] and all(np.isfinite(by_events[0])) and by_events[0][0] != by_events[0][1]
    assert all(torch.equal(a, b) for a, b in zip(by_events[1], by_frames[1]))


def test_train_events_tool_runs_two_steps(tmp_path):
    _gpu()
    rng = np.random.default_rng(0)
    H, W = SIZE
    n_lr = 64 * 14 + 1
    rec = {"lr_size": np.asarray(SIZE), "gt_size": np.asarray(GSIZE)}
    for side, n, (h, w) in (("lr", n_lr, SIZE), ("gt", 16 * n_lr, GSIZE)):
        rec[side + "_xs"], rec[side + "_ys"] = rng.integers(0, w, n).astype(np.int16), rng.integers(0, h, n).astype(np.int16)
        rec[side + "_ps"], rec[side + "_ts"] = rng.choice([-1.0, 1.0], n), np.sort(rng.uniform(0, 1, n))
    path, out = str(tmp_path / "rec.npz"), str(tmp_path / "rows.json")
    np.savez(path, **rec)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_events.py"), path, "--steps", "2", "--batch", "2", "--L", "4",
                        "--window", "128", "--sliding", "64", "--n-c", "16", "--n-b", "2", "--augment", "--pause", "0.2,0.5",
                        "--noise", "0.1", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    import json
    rows = json.load(open(out))
    assert [r["step"] for r in rows] == [0, 1] and all(np.isfinite(r["loss"]) and r["encode_ms"] > 0 for r in rows)
    assert p.stdout.count("loss") == 2
