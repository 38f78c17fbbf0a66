"""Deployment recordings on the MI355X (infer.MultiStreamSR without ground truth; events on the sensor's clock:
csrc/slot_emit_timed.hip, bmc_slot_emit_clocked): the entry point byte for byte against the numpy restatement
(event_clock_ref.emit_clocked_np), against bmc_slot_emit_timed where the two must agree, both capacity rules, the argument
checks; whole sessions of clocked, ground-truth-free recordings against the restatement of their kept predictions; sessions
without and with some ground truth; evaluate_recordings; counts_to_events(spans=).  Every comparison is exact."""
import numpy as np
import pytest
import torch

from event_clock_ref import SPANS, block_spans_np, emit_clocked_np
from event_output_ref import quantise_np
from event_times_ref import emit_timed_np
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_multistream import SCALE, SEQN, _model
from test_gpu_event_slots import _columns, _dev
from test_gpu_event_output import SENT16, SENT8, _frames
from test_gpu_event_times import GUARD, SENTF, _check_timed_slot, _emit_timed_once

pytestmark = pytest.mark.gpu

SENTD = np.float64(-7.25e300)        # what the float64 time column holds before a run
VALUES = np.array([0.0, 0.0, -1.0, 1.0, 2.0, 3.0, 5.0, 4.0], np.float32)      # counts 1, 2, 3, 5 (and 4: the ties 1/2 = 2/4)


def _preds(rng, S, sH, sW):
    """Counts around 3 on most elements (40 x 64: more than 4 096 events, so more than one scatter block), some 255."""
    P = VALUES[rng.integers(0, len(VALUES), (S, 2, sH, sW))]
    P = np.where(rng.random(P.shape) > 0.6, P + 2.0 * (P > 0), P)
    P[:, 0, 0, 0], P[:, 1, -1, -1], P[:, 0, sH // 2, sW // 2] = 255.0, 300.0, 254.0
    return P.astype(np.float32)


def _emit_clocked_once(dev, preds, active, spans, base, caps, max_count, wcap):
    """One bmc_slot_emit_clocked call on preds [S,2,sH,sW] (numpy).  spans[s] = (t_first, t_last) or None (the slot's clock
    entry has no column: the float32 behaviour).  Every column -- both time columns of every slot too -- is a view into a
    sentinel-filled tensor with GUARD entries on both sides.  -> per slot (xs, ys, ps, ts32, ts64, index[2]) as numpy, the
    columns WITH their guards."""
    from bmc_hip import slots
    S, _, sH, sW = preds.shape
    nparts = slots.emit_parts(sH, sW)
    pred = torch.tensor(preds).to(dev)
    full = lambda c, v, dt: torch.full((max(c, 1) + 2 * GUARD,), v, dtype=dt, device=dev)
    cols = [(full(c, SENT16, torch.int16), full(c, SENT16, torch.int16), full(c, SENT8, torch.int8),
             full(c, float(SENTF), torch.float32), full(c, float(SENTD), torch.float64)) for c in caps]
    index = torch.tensor([[b, -1] for b in base], dtype=torch.int64).to(dev)
    parts = torch.zeros(S * nparts, dtype=torch.int32, device=dev)
    scratch = torch.empty(slots.emit_timed_scratch_bytes(S, nparts, wcap), dtype=torch.uint8, device=dev)
    table = slots.SlotTable(S, dev, emit=True, timed=True, clock=True)
    e, em, ck = table.host(), table.emit_host(), table.clock_host()
    for s in range(S):
        if not active[s]:
            continue
        e[s]["frames"], e[s]["flags"] = pred.data_ptr(), slots.ACTIVE
        for k, t in zip(("xs", "ys", "ps"), cols[s]):
            em[s][k] = t.data_ptr() + GUARD * t.element_size()
        em[s]["index_in"], em[s]["index_out"] = index[s].data_ptr(), index[s].data_ptr() + 8
        em[s]["capacity"] = caps[s]
        if spans[s] is None:
            em[s]["ts"] = cols[s][3].data_ptr() + 4 * GUARD
        else:
            ck[s]["t_first"], ck[s]["t_last"] = spans[s]
            ck[s]["ts"] = cols[s][4].data_ptr() + 8 * GUARD
    table.upload()
    before = slots.EMIT_TIMED_LAUNCHES
    slots.emit_clocked(table, pred, max_count, nparts, parts, scratch, wcap)
    assert slots.EMIT_TIMED_LAUNCHES == before + 1
    torch.cuda.synchronize()
    return [tuple(t.cpu().numpy() for t in cols[s]) + (index[s].cpu().numpy(),) for s in range(S)]


def _check_clocked_slot(got, P, span, emits, base, cap, max_count, wcap):
    """Columns (guards included), index: byte for byte.  The float32 column of a clocked slot keeps its sentinels."""
    xs, ys, ps, ts32, ts64, index = got
    if not emits:
        assert index.tolist() == [base, -1]
        for g, sent in zip((xs, ys, ps, ts32, ts64), (SENT16, SENT16, SENT8, SENTF, SENTD)):
            assert (g == sent).all()
        return 0
    wx, wy, wp, wt, _ = emit_clocked_np(P, span, max_count)
    n = len(wx)
    assert index.tolist() == [base, base + n]                          # the true count, past either capacity too
    k = max(0, min(n, cap - base)) if n <= wcap else 0                 # events that fit
    for g, w, sent in ((xs, wx, SENT16), (ys, wy, SENT16), (ps, wp, SENT8), (ts64, wt, SENTD)):
        want = np.full(len(g), sent, g.dtype)
        want[GUARD + base:GUARD + base + k] = w[:k]
        assert g.tobytes() == want.tobytes()
    assert (ts32 == SENTF).all()
    if k:
        assert (np.diff(ts64[GUARD + base:GUARD + base + k]) >= 0).all()
    return n


# ------------------------------------------------------------------ 1. the entry point, byte for byte
@pytest.mark.parametrize("sH,sW", [(5, 7), (40, 64)])
@pytest.mark.parametrize("S", [1, 3])
def test_clocked_emit_bit_exact(sH, sW, S):
    """A different span per slot (a degenerate one, epoch seconds, sensor microseconds, one microsecond); with S = 3 slot 1
    is empty.  Twice: identical bytes."""
    dev = _gpu()
    rng = np.random.default_rng(100 * sH + S)
    preds = _preds(rng, S, sH, sW)
    active = [s != 1 for s in range(S)]
    spans = [SPANS[(s + (sH > 5)) % len(SPANS)] for s in range(S)] if S > 1 else [SPANS[1 + (sH > 5)]]
    counts = [int(quantise_np(p).sum()) for p in preds]
    assert {1, 2, 3, 5, 255} <= set(quantise_np(preds[0]).ravel().tolist())
    if sH == 40:
        assert min(counts) > 4096                                      # more than one block of the scatter pass
    base = [3 + 7 * s for s in range(S)]
    caps = [base[s] + counts[s] + 11 for s in range(S)]
    wcap = max(counts) + 5
    runs = []
    for _ in range(2):
        got = _emit_clocked_once(dev, preds, active, spans, base, caps, 255, wcap)
        for s in range(S):
            n = _check_clocked_slot(got[s], preds[s], spans[s], active[s], base[s], caps[s], 255, wcap)
            assert n == (counts[s] if active[s] else 0)
        runs.append(b"".join(a.tobytes() for g in got for a in g))
    assert runs[0] == runs[1]


@pytest.mark.parametrize("span", SPANS)
def test_every_span_at_the_small_size(span):
    dev = _gpu()
    preds = _preds(np.random.default_rng(7), 1, 5, 7)
    n = int(quantise_np(preds[0]).sum())
    (got,) = _emit_clocked_once(dev, preds, [True], [span], [0], [n], 255, n)
    assert _check_clocked_slot(got, preds[0], span, True, 0, n, 255, n) == n
    ts = got[4][GUARD:GUARD + n]
    d = np.float64(span[1]) - np.float64(span[0])
    assert ts[0] == np.float64(span[0]) + 0.01 * d and ts[-1] == np.float64(span[0]) + d


# ------------------------------------------------------------------ 2. against bmc_slot_emit_timed
@pytest.mark.parametrize("sH,sW", [(5, 7), (40, 64)])
def test_unit_span_rounds_to_the_timed_column(sH, sW):
    """Span (0.0, 1.0): t = tau, and float32(tau) is bmc_slot_emit_timed's time bit for bit; xs / ys / ps are identical."""
    dev = _gpu()
    preds = _preds(np.random.default_rng(sH), 2, sH, sW)
    counts = [int(quantise_np(p).sum()) for p in preds]
    base, caps, wcap = [0, 5], [c + 9 for c in counts], max(counts)
    clocked = _emit_clocked_once(dev, preds, [True] * 2, [(0.0, 1.0)] * 2, base, caps, 255, wcap)
    timed = _emit_timed_once(dev, preds, [True] * 2, [True] * 2, base, caps, 255, wcap)
    for s in range(2):
        a, z = GUARD + base[s], GUARD + base[s] + min(counts[s], caps[s] - base[s])
        for k in range(3):
            assert clocked[s][k].tobytes() == timed[s][k].tobytes()
        assert clocked[s][4][a:z].astype(np.float32).tobytes() == timed[s][3][a:z].tobytes()
        assert clocked[s][5].tolist() == timed[s][4].tolist()


def test_a_slot_without_a_clock_column_gets_the_timed_bytes():
    """Slots 0 and 2 are clocked, slot 1's clock entry has ts == NULL: its bytes (float32 column included) equal those of a
    plain bmc_slot_emit_timed call, its float64 column is untouched; the neighbours equal the restatement."""
    dev = _gpu()
    preds = _preds(np.random.default_rng(11), 3, 40, 64)
    counts = [int(quantise_np(p).sum()) for p in preds]
    base, caps, wcap = [2, 9, 0], [c + 20 for c in counts], max(counts)
    spans = [SPANS[2], None, SPANS[1]]
    got = _emit_clocked_once(dev, preds, [True] * 3, spans, base, caps, 255, wcap)
    timed = _emit_timed_once(dev, preds, [True] * 3, [True] * 3, base, caps, 255, wcap)
    for k in range(4):
        assert got[1][k].tobytes() == timed[1][k].tobytes()
    assert (got[1][4] == SENTD).all() and got[1][5].tolist() == timed[1][4].tolist()
    _check_timed_slot(got[1][:4] + (got[1][5],), preds[1], True, base[1], caps[1], 255, wcap)
    for s in (0, 2):
        _check_clocked_slot(got[s], preds[s], spans[s], True, base[s], caps[s], 255, wcap)


# ------------------------------------------------------------------ 3. capacities, arguments
def test_capacity_rules_are_those_of_the_timed_output():
    """Slot 0's columns end inside its window: the events past `capacity` are dropped.  Slot 1's window is one event larger
    than window_capacity: nothing is stored.  The index advances by the true count in both; slot 2 is whole."""
    dev = _gpu()
    preds = _preds(np.random.default_rng(13), 3, 5, 7)
    preds[1, 0, :2, :] = 100.0                                         # slot 1 is the largest window by far
    counts = [int(quantise_np(p).sum()) for p in preds]
    assert counts[1] > max(counts[0], counts[2])
    base = [4, 0, 6]
    caps = [base[0] + counts[0] // 2, counts[1] + 10, base[2] + counts[2]]
    wcap = counts[1] - 1
    spans = [SPANS[1], SPANS[2], SPANS[3]]
    got = _emit_clocked_once(dev, preds, [True] * 3, spans, base, caps, 255, wcap)
    for s in range(3):
        assert _check_clocked_slot(got[s], preds[s], spans[s], True, base[s], caps[s], 255, wcap) == counts[s]
    assert (got[1][4] == SENTD).all() and got[1][5].tolist() == [0, counts[1]]
    kept = got[0][4][GUARD + base[0]:]
    assert (kept[:counts[0] // 2] != SENTD).all() and (kept[counts[0] // 2:] == SENTD).all()


def test_emit_clocked_refuses_bad_arguments():
    """Errors without a launch (the launch counter does not move)."""
    dev = _gpu()
    from bmc_hip import lib, slots
    pred = torch.zeros(2, 2, 8, 8, device=dev)
    parts = torch.zeros(8, dtype=torch.int32, device=dev)
    scratch = torch.zeros(slots.emit_timed_scratch_bytes(2, 1, 100), dtype=torch.uint8, device=dev)
    table = slots.SlotTable(2, dev, emit=True, timed=True, clock=True)
    before = slots.EMIT_TIMED_LAUNCHES
    with pytest.raises(ValueError, match="no clock entries"):
        slots.emit_clocked(slots.SlotTable(2, dev, emit=True, timed=True), pred, 255, 1, parts, scratch, 100)
    with pytest.raises(ValueError, match="clock=True needs timed=True"):
        slots.SlotTable(2, dev, emit=True, clock=True)
    with pytest.raises(ValueError, match="max_count"):
        slots.emit_clocked(table, pred, 256, 1, parts, scratch, 100)
    with pytest.raises(ValueError, match="scratch must be"):
        slots.emit_clocked(table, pred, 255, 1, parts, scratch, 101)
    with pytest.raises(ValueError, match="window_capacity"):
        slots.emit_clocked(table, pred, 255, 1, parts, scratch, 0)
    args = lambda clock, mc, wc: (table.ptr(), table.emit_ptr(), clock, 2, pred.data_ptr(), 8, 8, mc, 1, parts.data_ptr(),
                                  slots.emit_rank_table(dev).data_ptr(), scratch.data_ptr(), wc, None)
    with pytest.raises(RuntimeError, match="clock table"):             # ... and the library checks for itself
        lib.call(lib._slot_emit_clocked, "bmc_slot_emit_clocked", *args(None, 255, 100))
    with pytest.raises(RuntimeError, match="bmc_slot_emit_clocked: 1 <= max_count"):
        lib.call(lib._slot_emit_clocked, "bmc_slot_emit_clocked", *args(table.clock_ptr(), 256, 100))
    with pytest.raises(RuntimeError, match="window_capacity"):
        lib.call(lib._slot_emit_clocked, "bmc_slot_emit_clocked", *args(table.clock_ptr(), 255, 0))
    assert slots.EMIT_TIMED_LAUNCHES == before
    assert table.clock_ptr() == table.emit_ptr() + 2 * slots.SLOT_EMIT_TIMED_DTYPE.itemsize and table.clock_ptr() % 8 == 0


# ------------------------------------------------------------------ 4. sessions on the sensor's clock, without ground truth
def _clocked_recording(seed, n_windows, H, W, t0):
    """A synthetic LR event stream with float64 stamps from t0 on -> (lr columns, lr_ts, lr_index), numpy."""
    from bmc_hip.encodings import event_window_indices
    rng = np.random.default_rng(seed)
    window = 2 * H * W
    L = n_windows + SEQN - 1
    n_lr = (window // 2) * L + 7
    lr = _columns(rng, n_lr, H, W)
    lr_ts = t0 + np.sort(rng.uniform(0, 2.0, n_lr))
    lr_index, none = event_window_indices(lr_ts, None, window, window // 2, SCALE)
    assert none is None and len(lr_index) == L
    return lr, lr_ts, lr_index


def _check_clocked_stream(res, spans, max_count=255):
    xs, ys, ps = (t.cpu().numpy() for t in res["sr_events"])
    ts = res["sr_ts"].cpu().numpy()
    index = res["sr_index"].numpy()
    preds = res["predictions"].cpu().numpy()
    assert ts.dtype == np.float64 and len(ts) == len(xs) == index[-1] and len(index) == len(preds) + 1
    assert "esr_mse" not in res and "bicubic_mse" not in res and len(res["time"]) == len(preds)
    for i, P in enumerate(preds):
        wx, wy, wp, wt, q = emit_clocked_np(P, spans[i + 1], max_count)           # window i predicts item i + 1
        a, b = index[i], index[i + 1]
        assert b - a == len(wx), i
        assert xs[a:b].tobytes() == wx.tobytes() and ys[a:b].tobytes() == wy.tobytes() and ps[a:b].tobytes() == wp.tobytes(), i
        assert ts[a:b].tobytes() == wt.tobytes(), i
        assert (np.diff(ts[a:b]) >= 0).all()
        if b > a:
            assert spans[i + 1, 0] <= ts[a] and ts[b - 1] <= spans[i + 1, 0] + (spans[i + 1, 1] - spans[i + 1, 0])
    assert index[-1] > 0.05 * preds.size                               # a real stream
    return b"".join(a.tobytes() for a in (xs, ys, ps, ts, index))


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("plain", [False, True])
def test_clocked_session_without_ground_truth(plain, graph):
    """Three event-backed recordings of 2, 6 and 4 windows in 2 slots (a slot is handed over), opened with lr_ts (on the GPU,
    on the host) and without ground truth: no metrics launch, no result sums, a 1 x 1 ground-truth scratch."""
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(plain, n_c, seed=511).to(dev)
    ms = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE, plain=plain, graph=graph, keep_predictions=True, emit_events=True,
                       event_times="linear")
    hs, spans = [], []
    for k, n in enumerate([2, 6, 4]):
        lr, lr_ts, lr_index = _clocked_recording(520 + k, n, H, W, [1.7e9, 123456789.0, 0.0][k])
        col = torch.tensor(lr_ts).to(dev) if k % 2 == 0 else lr_ts
        hs.append(ms.open_events(_dev(lr, dev), None, lr_index, None, (H, W), None, lr_ts=col))
        spans.append(block_spans_np(lr_ts, lr_index))
        r = ms._recs[hs[-1]]
        assert r["ev_ts"].dtype == torch.float64 and "sse" not in r and r["spans"].tobytes() == spans[-1].tobytes()
        assert ms.resident_bytes(hs[-1]) == sum(t.numel() * t.element_size() for t in r["lr"] + (
            r["keep"], r["ev_xs"], r["ev_ys"], r["ev_ps"], r["ev_index"])) + 8 * r["ev_capacity"]
    before, timed = dict(slots.LAUNCHES), slots.EMIT_TIMED_LAUNCHES
    ms.run()
    steps = slots.LAUNCHES["stage"] - before["stage"]
    assert slots.LAUNCHES["metrics"] == before["metrics"] and (graph or steps == 6)
    assert slots.EMIT_TIMED_LAUNCHES > timed and ms._size == (H, W)
    if graph:
        assert ms._graph is not None and ms.replays > 0
    assert tuple(ms._bufs["gt_scratch"].shape) == (2, 2, 1, 1)
    assert ms.scratch_bytes() == slots.emit_timed_scratch_bytes(2, slots.emit_parts(SCALE * H, SCALE * W), ms._wcap) + \
        4 * 2 * (SEQN * 2 * H * W + 2)
    for h, sp in zip(hs, spans):
        _check_clocked_stream(ms.results(h), sp)


def test_clocked_and_unclocked_recordings_share_a_session():
    """Frame-backed, one with spans and one without: float64 on the clock and float32 inside the window, side by side."""
    dev = _gpu()
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=531).to(dev)
    (f0, g0), (f1, g1) = _frames(532, 3, H, W), _frames(533, 3, H, W)
    L = f0.shape[0]
    sp = np.stack([123456789.0 + 3048.0 * np.arange(L), 123456789.0 + 3048.0 * np.arange(L) + 3048.0], 1)
    ms = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE, keep_predictions=True, emit_events=True, event_times="linear")
    h0 = ms.open(f0.to(dev), g0.to(dev))
    ms.step()
    h1 = ms.open(f1.to(dev), spans=sp)                                 # the table grows a clock part mid-session
    ms.run()
    r0, r1 = ms.results(h0), ms.results(h1)
    assert r0["sr_ts"].dtype == torch.float32 and "esr_mse" in r0
    ts, index = r0["sr_ts"].cpu().numpy(), r0["sr_index"].numpy()
    for i, P in enumerate(r0["predictions"].cpu().numpy()):
        assert ts[index[i]:index[i + 1]].tobytes() == emit_timed_np(P)[3].tobytes(), i
    _check_clocked_stream(r1, sp)


# ------------------------------------------------------------------ 5. sessions without / with some ground truth
def test_frames_without_ground_truth():
    """The predictions are bit-identical to the same recordings opened WITH a ground truth (same slots); bmc_slot_metrics is
    never launched; results() carries no metric."""
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=541).to(dev)
    recs = [_frames(542 + k, n, H, W) for k, n in enumerate([3, 5, 2])]
    out = []
    for gt in (True, False):
        ms = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE, keep_predictions=True)
        hs = [ms.open(f.to(dev), g.to(dev) if gt else None) for f, g in recs]
        before = dict(slots.LAUNCHES)
        ms.run()
        moved = {k: slots.LAUNCHES[k] - before[k] for k in before}
        assert moved["stage"] == moved["commit"] == 5 and moved["metrics"] == (5 if gt else 0)
        out.append([ms.results(h) for h in hs])
        if not gt:
            assert ms._size == (H, W) and all("sse" not in ms._recs[h] for h in hs)
            assert ms.resident_bytes(hs[0]) == 4 * (recs[0][0].numel() + 3 * 2 * SCALE * H * SCALE * W) and ms.scratch_bytes() == 0
    for a, b in zip(*out):
        assert torch.equal(a["predictions"], b["predictions"])
        assert set(a) == {"esr_mse", "bicubic_mse", "time", "predictions"} and set(b) == {"time", "predictions"}
        assert len(b["time"]) == len(a["time"])


def test_mixed_session_metrics_and_recapture():
    """Graph mode, 2 slots.  Two recordings without ground truth run (no metrics launch; the window is captured); then one WITH
    ground truth is opened: the graph is dropped and captured again with the metrics launch, and the recording's esr_mse /
    bicubic_mse are bit-identical to those of a session that holds only it (the same slot)."""
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=551).to(dev)
    (a0, _), (a1, _), (f, g) = _frames(552, 3, H, W), _frames(553, 9, H, W), _frames(554, 4, H, W)
    solo = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE, graph=True, keep_predictions=True)
    hb = solo.open(f.to(dev), g.to(dev))
    solo.run()
    want = solo.results(hb)

    ms = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE, graph=True, keep_predictions=True)
    h0, h1 = ms.open(a0.to(dev)), ms.open(a1.to(dev))
    before = slots.LAUNCHES["metrics"]
    for _ in range(4):                                                 # a0 ends after 3 windows; the capture is in window 3
        assert ms.step()
    assert ms._graph is not None and ms.replays == 2 and slots.LAUNCHES["metrics"] == before and ms._size == (H, W)
    h = ms.open(f.to(dev), g.to(dev))                                  # the first recording with ground truth: slot 0
    assert ms._graph is None and ms._size == (H, W, SCALE * H, SCALE * W)
    ms.run()
    assert ms._graph is not None and slots.LAUNCHES["metrics"] == before + 1      # one capture; the replays launch nothing
    got = ms.results(h)
    assert got["esr_mse"] == want["esr_mse"] and got["bicubic_mse"] == want["bicubic_mse"] and len(got["esr_mse"]) == 4
    assert torch.equal(got["predictions"], want["predictions"])
    assert "esr_mse" not in ms.results(h0) and "esr_mse" not in ms.results(h1) and len(ms.results(h1)["time"]) == 9
    with pytest.raises(ValueError, match="differ"):                    # another ground-truth size is refused
        ms.open(f.to(dev), g[..., :-2].contiguous().to(dev))
    with pytest.raises(ValueError, match="differ"):                    # and so is another LR size, with or without one
        ms.open(torch.zeros(3, 2, H, W + 1, device=dev))


def test_evaluate_recordings_without_and_with_some_ground_truth():
    dev = _gpu()
    from infer import EventRecording, evaluate_recordings
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=561).to(dev)
    (f0, g0), (f1, g1) = _frames(562, 3, H, W), _frames(563, 2, H, W)
    lr, _, lr_index = _clocked_recording(564, 2, H, W, 0.0)
    ev = EventRecording(_dev(lr, dev), lr_index=lr_index, lr_size=(H, W))
    none = evaluate_recordings(m, {"a": (f0.to(dev), None), "e": ev}, 2, n_c=n_c, scale=SCALE)
    assert set(none["results"]) == {"esr_mse", "bicubic_mse", "time", "params"}
    assert none["results"]["esr_mse"] == {} and none["results"]["bicubic_mse"] == {}
    assert set(none["results"]["time"]) == set(none["results"]["params"]) == {"a", "e"} and set(none["mean"]) == {"time", "params"}
    mixed = evaluate_recordings(m, {"b": (f1.to(dev), g1.to(dev)), "a": (f0.to(dev), None), "e": ev}, 2, n_c=n_c, scale=SCALE,
                                gt_size=(SCALE * H, SCALE * W))
    only = evaluate_recordings(m, {"b": (f1.to(dev), g1.to(dev))}, 2, n_c=n_c, scale=SCALE)
    assert set(mixed["results"]["esr_mse"]) == set(mixed["results"]["bicubic_mse"]) == {"b"}
    assert set(mixed["results"]["time"]) == set(mixed["results"]["params"]) == {"a", "b", "e"}
    assert set(mixed["mean"]) == {"esr_mse", "bicubic_mse", "time", "params"}
    assert mixed["mean"]["esr_mse"] == mixed["results"]["esr_mse"]["b"] > 0 and mixed["mean"]["bicubic_mse"] == mixed["results"]["bicubic_mse"]["b"]
    for k in ("esr_mse", "bicubic_mse"):                               # slot 0 in both sessions: the same bits
        assert mixed["results"][k]["b"] == only["results"][k]["b"]


# ------------------------------------------------------------------ 6. counts_to_events(spans=)
def test_counts_to_events_on_the_clock():
    dev = _gpu()
    from bmc_hip.encodings import counts_to_events
    B, sH, sW = 3, 6, 9
    preds = _preds(np.random.default_rng(61), B, sH, sW)
    preds[1] = 0.0
    spans = np.array([SPANS[1], SPANS[2], SPANS[3]])
    P = torch.tensor(preds).to(dev)
    plain = counts_to_events(P, times="linear")
    xs, ys, ps, ts, index = counts_to_events(P, times="linear", spans=spans)
    assert ts.dtype == torch.float64 and ts.is_cuda and torch.equal(index, plain[4]) and plain[3].dtype == torch.float32
    assert all(torch.equal(a, b) for a, b in zip((xs, ys, ps), plain[:3]))
    xs, ys, ps, ts, index = xs.cpu().numpy(), ys.cpu().numpy(), ps.cpu().numpy(), ts.cpu().numpy(), index.numpy()
    for b in range(B):
        wx, wy, wp, wt, _ = emit_clocked_np(preds[b], spans[b])
        a, z = index[b], index[b + 1]
        assert z - a == len(wx) and (b != 1 or z == a), b
        assert xs[a:z].tobytes() == wx.tobytes() and ys[a:z].tobytes() == wy.tobytes() and ps[a:z].tobytes() == wp.tobytes(), b
        assert ts[a:z].tobytes() == wt.tobytes(), b
    empty = counts_to_events(torch.full((2, 2, 8, 8), -1.0, device=dev), times="linear", spans=[[0.0, 1.0], [2.0, 3.0]])
    assert len(empty) == 5 and empty[3].numel() == 0 and empty[3].dtype == torch.float64 and empty[4].tolist() == [0, 0, 0]
