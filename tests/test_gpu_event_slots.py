"""Event-backed multi-stream inference on the MI355X (infer.MultiStreamSR.open_events, csrc/slot_events.hip): recordings
handed over as raw event columns + index tables and encoded window by window in one launch for all slots, against the same
recordings handed over as frames that the existing raw-column encoder (ops.encode_raw_events) made -- bit for bit."""
import numpy as np
import pytest
import torch

from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_multistream import SCALE, SEQN, _model

pytestmark = pytest.mark.gpu

WINDOW, SLIDING = 64, 32          # LR blocks of 64 events advancing by 32; ground-truth blocks of SCALE^2 * 64


# ------------------------------------------------------------------ helpers
def _columns(rng, n, h, w, hot=0):
    """Raw columns with a few events outside the sensor (both polarities), some p = 0 and, with hot, one pixel that `hot`
    events in a row hit."""
    xs = rng.integers(0, w, n).astype(np.int16)
    ys = rng.integers(0, h, n).astype(np.int16)
    ps = rng.choice([-1.0, 1.0], n)
    bad = rng.choice(n, max(n // 60, 8), replace=False)
    q = len(bad) // 4
    xs[bad[:q]] = w + rng.integers(0, 3, q)
    xs[bad[q:2 * q]] = -1 - rng.integers(0, 3, q)
    ys[bad[2 * q:3 * q]] = h + rng.integers(0, 3, q)
    ys[bad[3 * q:]] = -1 - rng.integers(0, 3, len(bad) - 3 * q)
    ps[bad[::2]] = -1.0                                    # out-of-range negatives: they count at [H-1, 0] of channel 1
    ps[bad[1::2]] = 1.0                                    # out-of-range positives: they count nowhere
    ps[rng.choice(n, max(n // 200, 2), replace=False)] = 0.0
    if hot:
        a = n // 3
        xs[a:a + hot], ys[a:a + hot] = w // 2, h // 3
        ps[a:a + hot] = rng.choice([-1.0, 1.0], hot)
    return xs, ys, ps


def _dev(cols, dev):
    return tuple(torch.tensor(c).to(dev) for c in cols)


def _recording(seed, n_windows, H, W, gh, gw):
    """A synthetic event recording of n_windows windows -> (lr columns, gt columns, lr_index, gt_index), numpy; the tables
    come from event_window_indices (tail blocks clamped, the last ground-truth blocks moved back)."""
    from bmc_hip.encodings import event_window_indices
    rng = np.random.default_rng(seed)
    L = n_windows + SEQN - 1
    n_lr = (WINDOW - SLIDING) * L + 7
    n_gt = SCALE * SCALE * n_lr
    lr, gt = _columns(rng, n_lr, H, W), _columns(rng, n_gt, gh, gw)
    lr_ts, gt_ts = np.sort(rng.uniform(0, 1, n_lr)), np.sort(rng.uniform(0, 1, n_gt))
    lr_index, gt_index = event_window_indices(lr_ts, gt_ts, WINDOW, SLIDING, SCALE)
    assert len(lr_index) == len(gt_index) == L
    return lr, gt, lr_index, gt_index


def _encode_frames(cols, index, h, w, dev):
    """frames[j] = the existing raw-column encoder (no flips) on columns[index[j,0]:index[j,1]] -> [L,2,h,w] on the GPU."""
    from bmc_hip import ops
    idx = np.concatenate([np.arange(a, b) for a, b in index] or [np.zeros(0, np.int64)])
    off = np.concatenate([[0], np.cumsum(index[:, 1] - index[:, 0])]).astype(np.int64)
    xs, ys, ps = (torch.tensor(np.ascontiguousarray(c[idx])).to(dev) for c in cols)
    return ops.encode_raw_events(xs, ys, ps, torch.tensor(off).to(dev), None, h, w)


def _session(m, n_c, plain, S, graph, keep=True):
    from infer import MultiStreamSR
    return MultiStreamSR(m, S, n_c=n_c, scale=SCALE, plain=plain, graph=graph, keep_predictions=keep)


def _same(a, b):
    assert a["esr_mse"] == b["esr_mse"] and a["bicubic_mse"] == b["bicubic_mse"]
    assert len(a["esr_mse"]) == a["predictions"].shape[0] == b["predictions"].shape[0] > 0
    assert torch.equal(a["predictions"], b["predictions"])


# ------------------------------------------------------------------ 1. the encode kernel on its own
@pytest.mark.parametrize("H,W,gh,gw,n_gt_block", [(10, 16, 40, 64, 1024), (31, 56, 124, 222, 2048), (180, 240, 720, 960, 32768)])
def test_slot_encode_bit_exact(H, W, gh, gw, n_gt_block):
    """S = 5, slots 1 and 3 without an event entry (their scratch keeps its sentinel).  Every LR and ground-truth scratch frame
    equals oracle.encode_raw_frame_np bit for bit: events outside the sensor of both polarities, a pixel hit by thousands of
    events, an empty range, ranges that overlap between the frames of a window and start at odd offsets; twice, same bytes."""
    dev = _gpu()
    from bmc_hip import slots
    from oracle import bmc_oracle as O
    S, with_entry = 5, (0, 2, 4)
    rng = np.random.default_rng(101 + H)
    n_lr, n_gt = 3 * 2048 + 11, 2 * n_gt_block + 13
    cols, dcols, ranges = {}, {}, {}
    for s in with_entry:
        cols[s] = (_columns(rng, n_lr, H, W, hot=3000), _columns(rng, n_gt, gh, gw, hot=5000 if n_gt_block > 8000 else 300))
        dcols[s] = (_dev(cols[s][0], dev), _dev(cols[s][1], dev))
        a = 3 + 2 * s
        lr_r = [(a, a + 2048), (a + 1024 + 1, a + 1024 + 1 + 2048), (a + 2048, min(a + 4096, n_lr))]     # overlapping, odd starts
        if s == 2:
            lr_r[2] = (777, 777)                                                                         # an empty range
        ranges[s] = (lr_r, (s + 1, s + 1 + n_gt_block))
    lr_scratch = torch.full((S, SEQN, 2, H, W), -7.0, device=dev)
    gt_scratch = torch.full((S, 2, gh, gw), -7.0, device=dev)
    table = slots.SlotTable(S, dev, events=True)

    def run():
        table.host()
        ev = table.events_host()
        for s in with_entry:
            for k, t in zip(("lr_xs", "lr_ys", "lr_ps", "gt_xs", "gt_ys", "gt_ps"), dcols[s][0] + dcols[s][1]):
                ev[k][s] = t.data_ptr()
            ev["lr_range"][s, :SEQN] = ranges[s][0]
            ev["gt_range"][s] = ranges[s][1]
        table.upload()
        before = slots.ENCODE_LAUNCHES
        slots.encode(table, lr_scratch, gt_scratch)
        assert slots.ENCODE_LAUNCHES == before + 1
        return lr_scratch.cpu().numpy().copy(), gt_scratch.cpu().numpy().copy()

    lr1, gt1 = run()
    for s in range(S):
        if s not in with_entry:
            assert (lr1[s] == -7.0).all() and (gt1[s] == -7.0).all(), s
            continue
        (lx, ly, lp), (gx, gy, gp) = cols[s]
        for t, (a, b) in enumerate(ranges[s][0]):
            want = O.encode_raw_frame_np(lx[a:b], ly[a:b], lp[a:b], 0, (H, W))
            assert np.array_equal(lr1[s, t], want), (s, t)
        a, b = ranges[s][1]
        want = O.encode_raw_frame_np(gx[a:b], gy[a:b], gp[a:b], 0, (gh, gw))
        assert want.max() >= 100 and want[1, gh - 1, 0] > 0           # the hot pixel and the out-of-range quirk are in there
        assert np.array_equal(gt1[s], want), s
    assert (lr1[2, 2] == 0).all()                                      # the empty range: an all-zero frame, written
    lr_scratch.fill_(-7.0)
    gt_scratch.fill_(-7.0)
    lr2, gt2 = run()
    assert lr1.tobytes() == lr2.tobytes() and gt1.tobytes() == gt2.tobytes()


def test_encode_refuses_bad_arguments():
    dev = _gpu()
    from bmc_hip import slots
    lr, gt = torch.zeros(2, SEQN, 2, 4, 8, device=dev), torch.zeros(2, 2, 16, 32, device=dev)
    with pytest.raises(ValueError):
        slots.encode(slots.SlotTable(2, dev), lr, gt)                  # a table without event entries
    table = slots.SlotTable(2, dev, events=True)
    with pytest.raises(ValueError):
        slots.encode(table, lr[:, :, :1], gt)
    with pytest.raises(ValueError):
        slots.encode(table, torch.zeros(2, 9, 2, 4, 8, device=dev), gt)
    with pytest.raises(ValueError):
        slots.encode(table, lr, torch.zeros(2, 2, 2, 7682, device=dev))


# ------------------------------------------------------------------ 2. end to end: the same as the frame-backed run
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("plain", [False, True])
def test_event_backed_equals_frame_backed(plain, graph, S):
    """6 recordings of 2-6 windows: slots are reused mid-run.  EventZoom-like ground truth two columns narrower than the
    prediction (the resize branch of the metrics)."""
    dev = _gpu()
    n_c, H, W = 16, 10, 16
    gh, gw = SCALE * H, SCALE * W - 2
    m = _model(plain, n_c, seed=111).to(dev)
    recs = [_recording(120 + k, n, H, W, gh, gw) for k, n in enumerate([3, 6, 2, 5, 4, 3])]
    by_frames = _session(m, n_c, plain, S, graph)
    hf = [by_frames.open(_encode_frames(lr, li, H, W, dev), _encode_frames(gt, gi, gh, gw, dev)) for lr, gt, li, gi in recs]
    by_frames.run()
    by_events = _session(m, n_c, plain, S, graph)
    he = [by_events.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (gh, gw)) for lr, gt, li, gi in recs]
    by_events.run()
    if graph:
        assert by_events._graph is not None and by_events.replays == by_frames.replays > 0
    for a, b, r in zip(he, hf, recs):
        ra, rb = by_events.results(a), by_frames.results(b)
        assert len(ra["esr_mse"]) == len(r[2]) - SEQN + 1
        _same(ra, rb)


@pytest.mark.parametrize("graph", [False, True])
def test_mixed_session(graph):
    """Two frame-backed and two event-backed recordings in one session of 3 slots == the all-frames session."""
    dev = _gpu()
    n_c, H, W = 16, 10, 16
    gh, gw = SCALE * H, SCALE * W
    m = _model(False, n_c, seed=131).to(dev)
    recs = [_recording(140 + k, n, H, W, gh, gw) for k, n in enumerate([4, 6, 3, 5])]
    frames = [(_encode_frames(lr, li, H, W, dev), _encode_frames(gt, gi, gh, gw, dev)) for lr, gt, li, gi in recs]
    ref = _session(m, n_c, False, 3, graph)
    hr = [ref.open(f, g) for f, g in frames]
    ref.run()
    ms = _session(m, n_c, False, 3, graph)
    hs = []
    for k, (lr, gt, li, gi) in enumerate(recs):
        if k % 2:
            hs.append(ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (gh, gw)))
        else:
            hs.append(ms.open(*frames[k]))
    ms.run()
    for a, b in zip(hs, hr):
        _same(ms.results(a), ref.results(b))
    with pytest.raises(ValueError):                                    # sizes must agree, whatever the kind
        ms.open_events(_dev(recs[0][0], dev), _dev(recs[0][1], dev), recs[0][2], recs[0][3], (H, W + 1), (gh, gw))


def test_open_events_refuses_fractional_polarities():
    dev = _gpu()
    lr, gt, li, gi = _recording(150, 2, 10, 16, 40, 64)
    lr = (lr[0], lr[1], lr[2] * 0.5)
    ms = _session(_model(False, 16).to(dev), 16, False, 2, False)
    with pytest.raises(ValueError, match="polarities"):
        ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (10, 16), (40, 64))


# ------------------------------------------------------------------ 3. evaluate_recordings
def test_evaluate_recordings_on_event_items():
    dev = _gpu()
    from infer import EventRecording, evaluate_recordings
    n_c, H, W = 16, 10, 16
    gh, gw = SCALE * H, SCALE * W
    m = _model(False, n_c, seed=151).to(dev)
    recs = {"r%d" % k: _recording(160 + k, n, H, W, gh, gw) for k, n in enumerate([3, 5, 2])}
    by_frames = {k: (_encode_frames(lr, li, H, W, dev), _encode_frames(gt, gi, gh, gw, dev)) for k, (lr, gt, li, gi) in recs.items()}
    by_events = {k: EventRecording(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (gh, gw)) for k, (lr, gt, li, gi) in recs.items()}
    kw = dict(n_c=n_c, scale=SCALE, gt_size=(gh, gw), keep_predictions=True)
    a, b = evaluate_recordings(m, by_events, 2, **kw), evaluate_recordings(m, by_frames, 2, **kw)
    for out in (a, b):
        out["results"].pop("time")
        out["mean"].pop("time")
    assert a["results"] == b["results"] and a["mean"] == b["mean"]
    assert all(torch.equal(a["predictions"][k], b["predictions"][k]) for k in recs)
    mixed = evaluate_recordings(m, [by_events["r0"], by_frames["r1"]], 2, n_c=n_c, scale=SCALE)
    assert mixed["results"]["esr_mse"] == {"0": a["results"]["esr_mse"]["r0"], "1": a["results"]["esr_mse"]["r1"]}
    with pytest.raises(ValueError):
        evaluate_recordings(m, by_events, 2, n_c=n_c, scale=SCALE, gt_size=(gh, gw - 2))


# ------------------------------------------------------------------ 4. launch accounting
def test_launches_per_window():
    dev = _gpu()
    from bmc_hip import slots
    n_c, H, W = 16, 10, 16
    gh, gw = SCALE * H, SCALE * W
    m = _model(False, n_c, seed=171).to(dev)
    recs = [_recording(180 + k, 8, H, W, gh, gw) for k in range(4)]
    frames = [(_encode_frames(lr, li, H, W, dev), _encode_frames(gt, gi, gh, gw, dev)) for lr, gt, li, gi in recs]
    keys = set(slots.LAUNCHES)
    assert keys == {"stage", "commit", "metrics"}

    def deltas(ms):
        before, enc = dict(slots.LAUNCHES), slots.ENCODE_LAUNCHES
        assert ms.step()
        return {k: slots.LAUNCHES[k] - before[k] for k in before}, slots.ENCODE_LAUNCHES - enc

    one = {"stage": 1, "commit": 1, "metrics": 1}
    none = {"stage": 0, "commit": 0, "metrics": 0}
    # eager, event-backed: one of each per window, encode included
    ms = _session(m, n_c, False, 2, False, keep=False)
    for lr, gt, li, gi in recs[:2]:
        ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (gh, gw))
    for _ in range(3):
        assert deltas(ms) == (one, 1)
    # eager, frames only: no encode launch, no scratch, the same keys as ever
    ms = _session(m, n_c, False, 2, False, keep=False)
    for f, g in frames[:2]:
        ms.open(f, g)
    for _ in range(3):
        assert deltas(ms) == (one, 0)
    assert set(slots.LAUNCHES) == keys and ms.scratch_bytes() == 0 and "lr_scratch" not in ms._bufs
    # graph, frames only, then the first event-backed recording arrives after the capture
    def late(events):
        """Two frame-backed recordings; recordings 2 and 3 join after windows 4 and 7, event-backed or as frames."""
        ms = _session(m, n_c, False, 4, True, keep=True)
        hs = [ms.open(f, g) for f, g in frames[:2]]
        for _ in range(3):                # two eager windows, the capture with the first replay
            ms.step()
        assert ms._graph is not None and ms.replays == 1
        assert deltas(ms) == (none, 0) and ms.replays == 2
        lr, gt, li, gi = recs[2]
        if events:
            hs.append(ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (gh, gw)))
            assert ms._graph is None      # the captured window has no encode launch: captured again at the next step
            assert deltas(ms) == (one, 1) and ms._graph is not None and ms.replays == 3
        else:
            hs.append(ms.open(*frames[2]))
            assert deltas(ms) == (none, 0) and ms.replays == 3
        for k in range(2):                # replays: the encode launch is inside the graph
            assert deltas(ms) == (none, 0) and ms.replays == 4 + k
        lr, gt, li, gi = recs[3]
        hs.append(ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (gh, gw)) if events else ms.open(*frames[3]))
        assert ms._graph is not None      # a second event-backed recording changes nothing
        before, enc = dict(slots.LAUNCHES), slots.ENCODE_LAUNCHES
        ms.run()
        assert slots.LAUNCHES == before and slots.ENCODE_LAUNCHES == enc
        assert ms.scratch_bytes() == (4 * 4 * (SEQN * 2 * H * W + 2 * gh * gw) if events else 0)
        return [ms.results(h) for h in hs]

    for x, y in zip(late(True), late(False)):       # ... and the late arrivals compute what they compute as frames
        _same(x, y)


# ------------------------------------------------------------------ 5. what a recording keeps on the GPU
@pytest.mark.parametrize("keep", [False, True])
def test_resident_bytes(keep):
    dev = _gpu()
    from bmc_hip import slots
    n_c, H, W = 16, 10, 16
    gh, gw = SCALE * H, SCALE * W - 2
    m = _model(False, n_c, seed=191).to(dev)
    lr, gt, li, gi = _recording(192, 5, H, W, gh, gw)
    L, nwin = len(li), 5
    ms = _session(m, n_c, False, 2, False, keep=keep)
    he = ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (gh, gw))
    hf = ms.open(_encode_frames(lr, li, H, W, dev), _encode_frames(gt, gi, gh, gw, dev))
    sums = nwin * slots.metric_parts(gh, gw) * 2 * 8
    kept = nwin * 2 * (SCALE * H) * (SCALE * W) * 4 if keep else 0
    assert ms.resident_bytes(he) == 12 * (len(lr[0]) + len(gt[0])) + sums + kept
    assert ms.resident_bytes(hf) == 4 * 2 * L * (H * W + gh * gw) + sums + kept
    assert ms.scratch_bytes() == 4 * 2 * (SEQN * 2 * H * W + 2 * gh * gw)
