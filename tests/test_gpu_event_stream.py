"""The continuous event stream on the MI355X (infer.MultiStreamSR(continuous=True); csrc/slot_emit_trimmed.hip,
bmc_slot_emit_trimmed; include/bmc_hip_stream.h): the entry point byte for byte against the numpy restatement
(event_stream_ref.emit_trimmed_np: the clocked window, then ts < t_cut), against bmc_slot_emit_clocked where nothing is cut, the
capacity rules on KEPT events, the argument checks; whole sessions with half-overlapping spans against the restatement of their
kept predictions and against the same session with the option off, trimmed on the host; self-ensemble; counts_to_events(cuts=).
Every comparison is exact."""
import numpy as np
import pytest
import torch

from event_clock_ref import SPANS, emit_clocked_np
from event_output_ref import quantise_np
from event_stream_ref import cuts_np, emit_trimmed_np, half_overlapping_spans, time_np
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_multistream import SCALE, SEQN, _model
from test_gpu_event_output import SENT16, SENT8, _frames
from test_gpu_event_times import GUARD, SENTF, _emit_timed_once
from test_gpu_event_clock import SENTD, _emit_clocked_once, _preds

pytestmark = pytest.mark.gpu

SENTQ = -4242                        # what a `dropped` word holds before a run


def _emit_trimmed_once(dev, preds, active, spans, cuts, base, caps, max_count, wcap, dropped=None):
    """One bmc_slot_emit_trimmed call on preds [S,2,sH,sW] (numpy).  spans[s] = (t_first, t_last) or None (the slot's clock entry
    has no column: untrimmed, float32); cuts[s]: the slot's t_cut; dropped[s] False: a NULL `dropped` pointer.  Every column is a
    view into a sentinel-filled tensor with GUARD entries on both sides.  -> per slot (xs, ys, ps, ts32, ts64, index[2], dropped
    word) as numpy, the columns WITH their guards."""
    from bmc_hip import slots, stream_lib
    S, _, sH, sW = preds.shape
    nparts = slots.emit_parts(sH, sW)
    pred = torch.tensor(preds).to(dev)
    full = lambda c, v, dt: torch.full((max(c, 1) + 2 * GUARD,), v, dtype=dt, device=dev)
    cols = [(full(c, SENT16, torch.int16), full(c, SENT16, torch.int16), full(c, SENT8, torch.int8),
             full(c, float(SENTF), torch.float32), full(c, float(SENTD), torch.float64)) for c in caps]
    index = torch.tensor([[b, -1] for b in base], dtype=torch.int64).to(dev)
    lost = torch.full((S,), SENTQ, dtype=torch.int64, device=dev)
    parts = torch.zeros(stream_lib.TRIM_PARTS * S * nparts, dtype=torch.int32, device=dev)
    scratch = torch.empty(slots.emit_timed_scratch_bytes(S, nparts, wcap), dtype=torch.uint8, device=dev)
    table = slots.SlotTable(S, dev, emit=True, timed=True, clock=True, trim=True)
    e, em, ck, tr = table.host(), table.emit_host(), table.clock_host(), table.trim_host()
    for s in range(S):
        tr[s]["t_cut"] = cuts[s]                                       # (an inactive slot has a cut too: nothing may read it)
        if dropped is None or dropped[s]:
            tr[s]["dropped"] = lost.data_ptr() + 8 * s
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
    slots.emit_trimmed(table, pred, max_count, nparts, parts, scratch, wcap)
    assert slots.EMIT_TIMED_LAUNCHES == before + 1
    torch.cuda.synchronize()
    lost = lost.cpu().numpy()
    return [tuple(t.cpu().numpy() for t in cols[s]) + (index[s].cpu().numpy(), int(lost[s])) for s in range(S)]


def _check_trimmed_slot(got, P, span, cut, emits, base, cap, max_count, wcap, has_dropped=True):
    """Columns (guards included: nothing past index_out is touched), index, dropped: byte for byte.  -> (kept, dropped)."""
    xs, ys, ps, ts32, ts64, index, lost = got
    if not emits:
        assert index.tolist() == [base, -1] and lost == SENTQ
        for g, sent in zip((xs, ys, ps, ts32, ts64), (SENT16, SENT16, SENT8, SENTF, SENTD)):
            assert (g == sent).all()
        return 0, 0
    wx, wy, wp, wt, dropped = emit_trimmed_np(P, span, cut, max_count)
    n = len(wx)
    assert index.tolist() == [base, base + n]                          # the KEPT count, past either capacity too
    assert lost == (dropped if has_dropped else SENTQ)
    k = max(0, min(n, cap - base)) if n <= wcap else 0                 # kept events that fit
    for g, w, sent in ((xs, wx, SENT16), (ys, wy, SENT16), (ps, wp, SENT8), (ts64, wt, SENTD)):
        want = np.full(len(g), sent, g.dtype)
        want[GUARD + base:GUARD + base + k] = w[:k]
        assert g.tobytes() == want.tobytes()
    assert (ts32 == SENTF).all()
    if k:
        assert (ts64[GUARD + base:GUARD + base + k] < cut).all()
    return n, dropped


def _cut(kind, span):
    t_first, d = np.float64(span[0]), np.float64(span[1]) - np.float64(span[0])
    return {"none": t_first + 0.01 * d, "all": np.inf, "mid": t_first + 0.37 * d, "half": time_np(1, 3, span)}[kind]


# ------------------------------------------------------------------ 1. the entry point, byte for byte
@pytest.mark.parametrize("kind", ["none", "all", "mid", "half"])
@pytest.mark.parametrize("sH,sW", [(5, 7), (40, 64)])
@pytest.mark.parametrize("S", [1, 3])
def test_trimmed_emit_bit_exact(sH, sW, S, kind):
    """S = 3: slot 0 is trimmed, slot 1 inactive, slot 2's clock entry has no column -- it gets bmc_slot_emit_timed's bytes,
    float32 column included, and dropped = 0.  "none": a cut at the window's earliest time, nothing is kept; "all": +inf, the
    bytes of bmc_slot_emit_clocked on the same inputs; "mid"; "half": exactly the time of rational 1/2, whose run of ties is
    dropped whole.  Twice: identical bytes."""
    dev = _gpu()
    rng = np.random.default_rng(100 * sH + S)
    preds = _preds(rng, S, sH, sW)
    active = [s != 1 for s in range(S)]
    spans = [SPANS[1 + (sH > 5)], None, None][:S]
    cuts = [_cut(kind, SPANS[1 + (sH > 5)])] * S
    counts = [int(quantise_np(p).sum()) for p in preds]
    assert {1, 2, 3, 5, 255} <= set(quantise_np(preds[0]).ravel().tolist())
    base = [3 + 7 * s for s in range(S)]
    caps = [base[s] + counts[s] + 11 for s in range(S)]
    wcap = max(counts) + 5
    runs = []
    for _ in range(2):
        got = _emit_trimmed_once(dev, preds, active, spans, cuts, base, caps, 255, wcap)
        kept, dropped = _check_trimmed_slot(got[0], preds[0], spans[0], cuts[0], True, base[0], caps[0], 255, wcap)
        assert kept + dropped == counts[0]
        assert {"none": kept == 0, "all": dropped == 0, "mid": 0 < kept < counts[0], "half": 0 < kept < counts[0]}[kind]
        if sH == 40 and kind in ("mid", "half"):
            assert kept > 4096                                         # more than one block of the scatter pass
        runs.append(b"".join(np.asarray(a).tobytes() for g in got for a in g))
    assert runs[0] == runs[1]
    if kind == "half":
        full = emit_clocked_np(preds[0], spans[0])[3]
        assert (full == cuts[0]).sum() > 1 and not (got[0][4] == cuts[0]).any()       # the tie run on the cut: all of it gone
    if kind == "all":
        clocked = _emit_clocked_once(dev, preds, active, spans, base, caps, 255, wcap)
        for s in range(S):
            assert all(got[s][k].tobytes() == clocked[s][k].tobytes() for k in range(6)), s
    if S == 3:
        _check_trimmed_slot(got[1], preds[1], None, cuts[1], False, base[1], caps[1], 255, wcap)
        timed = _emit_timed_once(dev, preds, active, [True] * 3, base, caps, 255, wcap)
        assert all(got[2][k].tobytes() == timed[2][k].tobytes() for k in range(4))
        assert (got[2][4] == SENTD).all() and got[2][5].tolist() == timed[2][4].tolist() == [base[2], base[2] + counts[2]]
        assert got[2][6] == 0


@pytest.mark.parametrize("span", [SPANS[0], (5.0e5, 5.0e5)])
def test_degenerate_span_is_kept_or_dropped_whole(span):
    """t_last == t_first: every event has t = t_first.  Slot 0's cut is t_first (all dropped), slot 1's the next float64 (all
    kept, the clocked bytes); slot 1 has no `dropped` pointer."""
    dev = _gpu()
    preds = _preds(np.random.default_rng(17), 2, 5, 7)
    counts = [int(quantise_np(p).sum()) for p in preds]
    cuts = [np.float64(span[0]), np.nextafter(np.float64(span[0]), np.inf)]
    base, caps, wcap = [2, 0], [c + 9 for c in counts], max(counts)
    got = _emit_trimmed_once(dev, preds, [True] * 2, [span] * 2, cuts, base, caps, 255, wcap, dropped=[True, False])
    assert _check_trimmed_slot(got[0], preds[0], span, cuts[0], True, base[0], caps[0], 255, wcap) == (0, counts[0])
    assert _check_trimmed_slot(got[1], preds[1], span, cuts[1], True, base[1], caps[1], 255, wcap, has_dropped=False) == (counts[1], 0)
    assert (got[0][4] == SENTD).all() and (got[1][4][GUARD:GUARD + counts[1]] == span[0]).all()


# ------------------------------------------------------------------ 2. capacities, arguments
def test_capacity_rules_apply_to_the_kept_events():
    """Slot 0's FULL count exceeds window_capacity, its kept count fits: stored.  Slot 1's kept count exceeds it: nothing is
    stored, the index advances by the kept count, dropped is still written.  Slot 2's columns end inside its kept events:
    positions at or beyond `capacity` are dropped."""
    dev = _gpu()
    preds = _preds(np.random.default_rng(13), 3, 5, 7)
    preds[1, 0, :2, :] = 100.0                                         # slot 1 is the largest window by far
    spans = [SPANS[1], SPANS[2], SPANS[3]]
    cuts = [_cut("mid", spans[0]), _cut("mid", spans[1]), _cut("mid", spans[2])]
    counts = [int(quantise_np(p).sum()) for p in preds]
    kept = [len(emit_trimmed_np(preds[s], spans[s], cuts[s])[0]) for s in range(3)]
    wcap = kept[1] - 1
    assert counts[0] > wcap >= kept[0] and kept[1] > wcap >= kept[2] > 8
    base = [4, 0, 6]
    caps = [base[0] + kept[0] + 3, counts[1] + 10, base[2] + kept[2] // 2]
    got = _emit_trimmed_once(dev, preds, [True] * 3, spans, cuts, base, caps, 255, wcap)
    for s in range(3):
        assert _check_trimmed_slot(got[s], preds[s], spans[s], cuts[s], True, base[s], caps[s], 255, wcap) == (kept[s], counts[s] - kept[s])
    assert (got[0][4][GUARD + base[0]:GUARD + base[0] + kept[0]] != SENTD).all()
    assert (got[1][4] == SENTD).all() and got[1][5].tolist() == [0, kept[1]] and got[1][6] == counts[1] - kept[1]
    tail = got[2][4][GUARD + base[2]:]
    assert (tail[:kept[2] // 2] != SENTD).all() and (tail[kept[2] // 2:] == SENTD).all()


def test_emit_trimmed_refuses_bad_arguments():
    """Errors without a launch (the launch counter does not move)."""
    dev = _gpu()
    from bmc_hip import lib, slots, stream_lib
    pred = torch.zeros(2, 2, 8, 8, device=dev)
    parts = torch.zeros(8, dtype=torch.int32, device=dev)
    scratch = torch.zeros(slots.emit_timed_scratch_bytes(2, 1, 100), dtype=torch.uint8, device=dev)
    table = slots.SlotTable(2, dev, emit=True, timed=True, clock=True, trim=True)
    before = slots.EMIT_TIMED_LAUNCHES
    with pytest.raises(ValueError, match="no trim entries"):
        slots.emit_trimmed(slots.SlotTable(2, dev, emit=True, timed=True, clock=True), pred, 255, 1, parts, scratch, 100)
    with pytest.raises(ValueError, match="trim=True needs clock=True"):
        slots.SlotTable(2, dev, emit=True, timed=True, trim=True)
    with pytest.raises(ValueError, match="max_count"):
        slots.emit_trimmed(table, pred, 256, 1, parts, scratch, 100)
    with pytest.raises(ValueError, match="scratch must be"):
        slots.emit_trimmed(table, pred, 255, 1, parts, scratch, 101)
    with pytest.raises(ValueError, match="window_capacity"):
        slots.emit_trimmed(table, pred, 255, 1, parts, scratch, 0)
    with pytest.raises(ValueError, match="2 \\* S \\* nparts"):         # kept and dropped totals
        slots.emit_trimmed(table, pred, 255, 1, parts[:3], scratch, 100)
    args = lambda clock, trim, mc, wc: (table.ptr(), table.emit_ptr(), clock, trim, 2, pred.data_ptr(), 8, 8, mc, 1, parts.data_ptr(),
                                        slots.emit_rank_table(dev).data_ptr(), scratch.data_ptr(), wc, None)
    call = lambda *a: lib.call(stream_lib._slot_emit_trimmed, "bmc_slot_emit_trimmed", *args(*a))
    with pytest.raises(RuntimeError, match="trim table"):              # ... and the library checks for itself
        call(table.clock_ptr(), None, 255, 100)
    with pytest.raises(RuntimeError, match="trim table"):
        call(table.clock_ptr(), table.trim_ptr() + 4, 255, 100)
    with pytest.raises(RuntimeError, match="clock table"):
        call(None, table.trim_ptr(), 255, 100)
    with pytest.raises(RuntimeError, match="bmc_slot_emit_trimmed: 1 <= max_count"):
        call(table.clock_ptr(), table.trim_ptr(), 256, 100)
    with pytest.raises(RuntimeError, match="window_capacity"):
        call(table.clock_ptr(), table.trim_ptr(), 255, 0)
    with pytest.raises(RuntimeError, match="window_capacity"):
        call(table.clock_ptr(), table.trim_ptr(), 255, (1 << 28) + 1)
    assert slots.EMIT_TIMED_LAUNCHES == before
    assert table.trim_ptr() == table.clock_ptr() + 2 * slots.SLOT_CLOCK_DTYPE.itemsize and table.trim_ptr() % 8 == 0


# ------------------------------------------------------------------ 3. sessions
H, W, N_C = 8, 12, 16
WINDOWS = [5, 3, 4]                  # three recordings in 2 slots: a slot is handed over


def _session(dev, m, plain, graph, spans, recs, continuous, self_ensemble=None, slots=2):
    from infer import MultiStreamSR
    ms = MultiStreamSR(m, slots, n_c=N_C, scale=SCALE, plain=plain, graph=graph, keep_predictions=True, emit_events=True,
                       event_times="linear", continuous=continuous, self_ensemble=self_ensemble)
    hs = [ms.open(f.to(dev), spans=sp) for (f, _), sp in zip(recs, spans)]
    ms.run()
    return ms, [ms.results(h) for h in hs]


def _np(res):
    xs, ys, ps = (t.cpu().numpy() for t in res["sr_events"])
    return xs, ys, ps, res["sr_ts"].cpu().numpy(), res["sr_index"].numpy()


def _check_continuous_stream(res, spans):
    """Every window's slice against the restatement on that window's kept prediction; the index, the dropped counts; the whole
    time column in order.  -> the stream's bytes."""
    xs, ys, ps, ts, index = _np(res)
    preds = res["predictions"].cpu().numpy()
    cuts = cuts_np(spans, len(preds))
    assert ts.dtype == np.float64 and len(ts) == len(xs) == index[-1] and len(index) == len(preds) + 1
    assert isinstance(res["sr_dropped"], list) and len(res["sr_dropped"]) == len(preds)
    for i, P in enumerate(preds):
        wx, wy, wp, wt, dropped = emit_trimmed_np(P, spans[i + 1], cuts[i])          # window i predicts item i + 1
        a, b = index[i], index[i + 1]
        assert b - a == len(wx) and res["sr_dropped"][i] == dropped, i
        assert xs[a:b].tobytes() == wx.tobytes() and ys[a:b].tobytes() == wy.tobytes() and ps[a:b].tobytes() == wp.tobytes(), i
        assert ts[a:b].tobytes() == wt.tobytes(), i
    assert (np.diff(ts) >= 0).all() and index[-1] > 0.02 * preds.size
    assert ts[0] >= spans[1, 0] and ts[-1] <= spans[len(preds), 1]
    return b"".join(a.tobytes() for a in (xs, ys, ps, ts, index))


def _host_trim(res, spans):
    """What a user did before the option: the untrimmed stream, filtered window by window on the host."""
    xs, ys, ps, ts, index = _np(res)
    cuts = cuts_np(spans, len(index) - 1)
    keep = np.concatenate([ts[index[i]:index[i + 1]] < cuts[i] for i in range(len(cuts))])
    kept = np.array([0] + [int(keep[index[i]:index[i + 1]].sum()) for i in range(len(cuts))], np.int64).cumsum()
    return b"".join(a.tobytes() for a in (xs[keep], ys[keep], ps[keep], ts[keep], kept))


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("plain", [False, True])
def test_continuous_session_with_half_overlapping_spans(plain, graph):
    dev = _gpu()
    from bmc_hip import slots
    m = _model(plain, N_C, seed=611).to(dev)
    recs = [_frames(620 + k, n, H, W) for k, n in enumerate(WINDOWS)]
    spans = [half_overlapping_spans(n + SEQN - 1, t0, step) for n, t0, step in zip(WINDOWS, (1.7e9, 123456789.0, 0.0), (0.0165, 1524.0, 0.5))]
    before = slots.EMIT_TIMED_LAUNCHES
    on, got = _session(dev, m, plain, graph, spans, recs, True)
    assert slots.EMIT_TIMED_LAUNCHES > before and on._bufs["table"].trim and on._bufs["emit_parts"].numel() == 2 * 2 * on._nparts
    if graph:
        assert on._graph is not None and on.replays > 0
    off, plain_res = _session(dev, m, plain, graph, spans, recs, False)
    assert not off._bufs["table"].trim and off._bufs["table"].dev.numel() + 2 * 16 == on._bufs["table"].dev.numel()
    for r, p, sp in zip(got, plain_res, spans):
        assert torch.equal(r["predictions"], p["predictions"]) and "sr_dropped" not in p
        stream = _check_continuous_stream(r, sp)
        assert stream == _host_trim(p, sp)                             # the option off, trimmed on the host: the same bytes
        assert not (np.diff(p["sr_ts"].cpu().numpy()) >= 0).all()      # ... which the untrimmed stream is not
        assert 0 < sum(r["sr_dropped"]) == int(p["sr_index"][-1] - r["sr_index"][-1]) and r["sr_dropped"][-1] == 0


def test_spans_that_do_not_overlap_change_nothing():
    dev = _gpu()
    m = _model(False, N_C, seed=631).to(dev)
    recs = [_frames(640 + k, n, H, W) for k, n in enumerate(WINDOWS[:2])]
    spans = []
    for n, t0 in zip(WINDOWS, (123456789.0, 5.0e5)):
        sp = half_overlapping_spans(n + SEQN - 1, t0, 1524.0)
        spans.append(np.stack([sp[:, 0], sp[:, 0] + 1523.0], 1))
    _, on = _session(dev, m, False, False, spans, recs, True)
    _, off = _session(dev, m, False, False, spans, recs, False)
    for a, b in zip(on, off):
        assert a["sr_dropped"] == [0] * len(a["sr_dropped"]) and torch.equal(a["sr_index"], b["sr_index"])
        assert torch.equal(a["sr_ts"], b["sr_ts"]) and all(torch.equal(x, y) for x, y in zip(a["sr_events"], b["sr_events"]))


def test_continuous_refusals_on_the_device_leave_no_trace():
    dev = _gpu()
    from infer import MultiStreamSR
    ms = MultiStreamSR(_model(True, N_C, seed=1).to(dev), 2, n_c=N_C, scale=SCALE, plain=True, emit_events=True, event_times="linear",
                       continuous=True)
    f = _frames(650, 3, H, W)[0].to(dev)
    bad = half_overlapping_spans(len(f), 10.0, 1.0)
    bad[2, 0] = 10.5                                                   # item 2 starts before item 1
    for kw in ({}, dict(spans=bad)):
        with pytest.raises(ValueError, match="no clock to cut on|t_first does not decrease"):
            ms.open(f, **kw)
        assert not ms._recs and ms._size is None and not ms.sched.pending()


def test_self_ensemble_trims_the_merged_prediction():
    dev = _gpu()
    m = _model(False, N_C, seed=661).to(dev)
    recs = [_frames(670 + k, n, H, W) for k, n in enumerate([3, 2])]
    spans = [half_overlapping_spans(n + SEQN - 1, 123456789.0 + 1e6 * k, 1524.0) for k, n in enumerate([3, 2])]
    ms, got = _session(dev, m, False, False, spans, recs, True, self_ensemble=2, slots=4)
    _, off = _session(dev, m, False, False, spans, recs, False, self_ensemble=2, slots=4)
    for r, p, sp in zip(got, off, spans):
        assert torch.equal(r["predictions"], p["predictions"])         # the leader's merged prediction is what is trimmed
        assert _check_continuous_stream(r, sp) == _host_trim(p, sp) and sum(r["sr_dropped"]) > 0


# ------------------------------------------------------------------ 4. counts_to_events(cuts=)
def test_counts_to_events_with_cuts():
    dev = _gpu()
    from bmc_hip.encodings import counts_to_events
    B, sH, sW = 4, 6, 9
    preds = _preds(np.random.default_rng(61), B, sH, sW)
    preds[1] = 0.0
    spans = np.array([SPANS[1], SPANS[2], SPANS[3], SPANS[2]])
    cuts = np.array([_cut("mid", spans[0]), np.inf, _cut("half", spans[2]), _cut("none", spans[3])])
    P = torch.tensor(preds).to(dev)
    xs, ys, ps, ts, index, dropped = counts_to_events(P, times="linear", spans=spans, cuts=cuts)
    assert ts.dtype == torch.float64 and ts.is_cuda and dropped.dtype == torch.int64 and not dropped.is_cuda
    xs, ys, ps, ts, index = xs.cpu().numpy(), ys.cpu().numpy(), ps.cpu().numpy(), ts.cpu().numpy(), index.numpy()
    for b in range(B):
        wx, wy, wp, wt, lost = emit_trimmed_np(preds[b], spans[b], cuts[b])
        a, z = index[b], index[b + 1]
        assert z - a == len(wx) and int(dropped[b]) == lost and (b not in (1, 3) or z == a), b
        assert xs[a:z].tobytes() == wx.tobytes() and ys[a:z].tobytes() == wy.tobytes() and ps[a:z].tobytes() == wp.tobytes(), b
        assert ts[a:z].tobytes() == wt.tobytes(), b
    assert len(ts) == index[-1] > 0 and int(dropped[3]) > 0 and int(dropped[1]) == 0
    whole = counts_to_events(P, times="linear", spans=spans, cuts=np.full(B, np.inf))
    plain = counts_to_events(P, times="linear", spans=spans)
    assert all(torch.equal(a, b) for a, b in zip(whole[:5], plain)) and whole[5].tolist() == [0] * B
    empty = counts_to_events(torch.full((2, 2, 8, 8), -1.0, device=dev), times="linear", spans=[[0.0, 1.0], [2.0, 3.0]], cuts=[0.5, 2.5])
    assert len(empty) == 6 and empty[3].numel() == 0 and empty[4].tolist() == [0, 0, 0] and empty[5].tolist() == [0, 0]
