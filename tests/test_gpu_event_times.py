"""Timed event output of multi-stream inference on the MI355X (infer.MultiStreamSR(emit_events=True, event_times="linear"),
csrc/slot_emit_timed.hip): the entry point byte for byte against the numpy restatement (event_times_ref.emit_timed_np), all
four columns; whole sessions against the restatement of their kept predictions, twice with identical bytes; the option off
changes nothing; both capacities; the launches per window; counts_to_events(times="linear")."""
import re

import numpy as np
import pytest
import torch

from event_output_ref import emit_np, quantise_np
from event_times_ref import emit_timed_np, times_np
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_multistream import SCALE, _model
from test_gpu_event_slots import _dev
from test_gpu_event_output import SENT16, SENT8, _event_recording, _frames, _synthetic, _with_silent_waves

pytestmark = pytest.mark.gpu

SENTF = np.float32(-7.25)            # what the time column holds before a run
GUARD = 64                           # sentinel entries in front of and behind every buffer the kernels write


def _emit_timed_once(dev, preds, active, entry, base, caps, max_count, wcap, nparts=None):
    """One bmc_slot_emit_timed call on preds [S,2,sH,sW] (numpy).  Every column is a view into a sentinel-filled tensor with
    GUARD entries on both sides; so is the sort scratch (bytes of 0xA5).  -> per slot (xs, ys, ps, ts, index[2]) as numpy, the
    columns WITH their guards."""
    from bmc_hip import slots
    S, _, sH, sW = preds.shape
    nparts = nparts or slots.emit_parts(sH, sW)
    pred = torch.tensor(preds).to(dev)
    full = lambda c, v, dt: torch.full((max(c, 1) + 2 * GUARD,), v, dtype=dt, device=dev)
    cols = [(full(c, SENT16, torch.int16), full(c, SENT16, torch.int16), full(c, SENT8, torch.int8),
             full(c, float(SENTF), torch.float32)) for c in caps]
    index = torch.tensor([[b, -1] for b in base], dtype=torch.int64).to(dev)
    parts = torch.zeros(S * nparts, dtype=torch.int32, device=dev)
    need = slots.emit_timed_scratch_bytes(S, nparts, wcap)
    scratch = torch.full((need + 2 * 8 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    table = slots.SlotTable(S, dev, emit=True, timed=True)
    e, em = table.host(), table.emit_host()
    for s in range(S):
        if active[s]:
            e[s]["frames"], e[s]["flags"] = pred.data_ptr(), slots.ACTIVE
        if entry[s]:
            for k, t in zip(("xs", "ys", "ps", "ts"), cols[s]):
                em[s][k] = t.data_ptr() + GUARD * t.element_size()
            em[s]["index_in"], em[s]["index_out"] = index[s].data_ptr(), index[s].data_ptr() + 8
            em[s]["capacity"] = caps[s]
    table.upload()
    before = slots.EMIT_TIMED_LAUNCHES
    slots.emit_timed(table, pred, max_count, nparts, parts, scratch[8 * GUARD:8 * GUARD + need], wcap)
    assert slots.EMIT_TIMED_LAUNCHES == before + 1
    torch.cuda.synchronize()
    sc = scratch.cpu().numpy()
    assert (sc[:8 * GUARD] == 0xA5).all() and (sc[8 * GUARD + need:] == 0xA5).all()       # nothing outside the scratch
    return [tuple(t.cpu().numpy() for t in cols[s]) + (index[s].cpu().numpy(),) for s in range(S)]


def _check_timed_slot(got, P, emits, base, cap, max_count, wcap):
    """Columns (guards included), index: byte for byte.  A window above wcap stores nothing and still counts."""
    *cols, index = got
    sents = (SENT16, SENT16, SENT8, SENTF)
    if not emits:
        assert index.tolist() == [base, -1]
        for g, sent in zip(cols, sents):
            assert (g == sent).all()
        return 0
    want_cols = emit_timed_np(P, max_count)[:4]
    n = len(want_cols[0])
    assert index.tolist() == [base, base + n]                          # the true count, past either capacity too
    for g, w, sent in zip(cols, want_cols, sents):
        want = np.full(len(g), sent, g.dtype)
        k = max(0, min(n, cap - base)) if n <= wcap else 0             # events that fit
        want[GUARD + base:GUARD + base + k] = w[:k]
        assert g.tobytes() == want.tobytes()
    return n


# ------------------------------------------------------------------ 1. the entry point, byte for byte
@pytest.mark.parametrize("sH,sW,S", [(36, 56, 1), (36, 56, 32), (124, 224, 3), (124, 224, 32), (720, 960, 1), (720, 960, 3),
                                     (37, 53, 3), (37, 53, 32)])
def test_timed_emit_bit_exact(sH, sW, S):
    """Synthetic predictions with every special value (as test_gpu_event_output); every 5th + 1 slot is inactive, every 5th + 3
    has no entry, slot 2 is all zero, one slot's column capacity ends inside its window; odd start positions."""
    dev = _gpu()
    rng = np.random.default_rng(2000 * sH + S)
    preds = np.stack([_synthetic(rng, sH, sW) for _ in range(S)])
    if S > 2:
        preds[2] = np.where(preds[2] > 0, -preds[2], preds[2])
        preds[2][np.isnan(preds[2])] = 0.0
    active = [s % 5 != 1 for s in range(S)]
    entry = [s % 5 != 3 for s in range(S)]
    counts = [int(quantise_np(p).sum()) for p in preds]
    base = [0 if s == 0 else 3 + 7 * s for s in range(S)]
    caps = [base[s] + counts[s] + 50 for s in range(S)]
    cut = S - 1 if S > 1 else None
    if cut is not None and (not active[cut] or not entry[cut] or counts[cut] < 10):
        cut = 0
    if cut is not None:
        caps[cut] = base[cut] + counts[cut] // 2 + 1
    wcap = max(counts) + 5
    runs = []
    for _ in range(2):
        got = _emit_timed_once(dev, preds, active, entry, base, caps, 255, wcap)
        total = 0
        for s in range(S):
            total += _check_timed_slot(got[s], preds[s], active[s] and entry[s], base[s], caps[s], 255, wcap)
        assert total > 0.2 * preds[0].size
        runs.append(b"".join(a.tobytes() for g in got for a in g))
    assert runs[0] == runs[1]
    if S > 2:
        assert got[2][4].tolist() == [base[2], base[2]]


@pytest.mark.parametrize("sH,sW,S", [(36, 56, 3), (124, 224, 1), (37, 53, 3)])
def test_all_zero_and_all_three(sH, sW, S):
    """Nothing at all; and every element equal to 3: three tie groups (j = 0, 1/2, 1) of 2*sH*sW events each, inside which the
    flat order must survive both digit passes."""
    dev = _gpu()
    zero = np.zeros((S, 2, sH, sW), np.float32)
    for g in _emit_timed_once(dev, zero, [True] * S, [True] * S, [4] * S, [10] * S, 255, 7):
        assert g[4].tolist() == [4, 4] and (g[0] == SENT16).all() and (g[3] == SENTF).all()
    three = np.full((S, 2, sH, sW), 3.0, np.float32)
    n = 6 * sH * sW
    got = _emit_timed_once(dev, three, [True] * S, [True] * S, [1] * S, [n + 1] * S, 255, n)
    for s in range(S):
        assert _check_timed_slot(got[s], three[s], True, 1, n + 1, 255, n) == n
    ts = got[0][3][GUARD + 1:GUARD + 1 + n]
    assert (ts[:n // 3] == np.float32(0.01)).all() and (ts[n // 3:2 * n // 3] == times_np([1], [3])[0]).all() and (ts[2 * n // 3:] == 1).all()


@pytest.mark.parametrize("max_count,value", [(255, 1000.0), (1, 0.7), (254, np.inf), (2, 2.5)])
def test_all_max_count_small(max_count, value):
    dev = _gpu()
    P = np.full((1, 2, 36, 56), value, np.float32)
    n = 2 * 36 * 56 * max_count
    (got,) = _emit_timed_once(dev, P, [True], [True], [5], [5 + n + 9], max_count, n)
    assert _check_timed_slot(got, P[0], True, 5, 5 + n + 9, max_count, n) == n


@pytest.mark.parametrize("nparts", [1, 2, 7, 64, 1024])
def test_any_number_of_parts_gives_the_same_timed_stream(nparts):
    dev = _gpu()
    rng = np.random.default_rng(nparts + 50)
    preds = np.stack([_synthetic(rng, 36, 56) for _ in range(3)])
    counts = [int(quantise_np(p).sum()) for p in preds]
    got = _emit_timed_once(dev, preds, [True] * 3, [True] * 3, [0, 11, 0], [c + 20 for c in counts], 255, max(counts), nparts=nparts)
    for s in range(3):
        _check_timed_slot(got[s], preds[s], True, [0, 11, 0][s], counts[s] + 20, 255, max(counts))


def test_a_wave_and_a_part_without_timed_events():
    """Zero wave totals in the tile scan of the expand launch and a zero part total (test_gpu_event_output states the layout)."""
    dev = _gpu()
    rng = np.random.default_rng(65)
    sH, sW, parts = 32, 96, 3
    P = _synthetic(rng, sH, sW)
    P = _with_silent_waves(np.where(quantise_np(P) > 0, P, np.float32(1.0)), parts)
    n = int(quantise_np(P).sum())
    (got,) = _emit_timed_once(dev, P[None], [True], [True], [3], [3 + n + 9], 255, n, nparts=parts)
    assert _check_timed_slot(got, P, True, 3, 3 + n + 9, 255, n) == n


def test_window_scratch_overflow_stores_nothing_and_counts():
    """Slot 1's window is one event larger than the sort scratch: its columns keep their sentinels, its index advances by the
    true count, the neighbours are whole, and no byte outside the scratch changes (the guards of _emit_timed_once)."""
    dev = _gpu()
    rng = np.random.default_rng(77)
    preds = np.stack([_synthetic(rng, 36, 56) for _ in range(3)])
    preds[1, 0, :8, :] = 100.0                                        # slot 1 is the largest window by far
    counts = [int(quantise_np(p).sum()) for p in preds]
    assert counts[1] > max(counts[0], counts[2])
    wcap = counts[1] - 1
    got = _emit_timed_once(dev, preds, [True] * 3, [True] * 3, [2, 3, 4], [c + 30 for c in counts], 255, wcap)
    for s in range(3):
        _check_timed_slot(got[s], preds[s], True, [2, 3, 4][s], counts[s] + 30, 255, wcap)
    assert (got[1][0] == SENT16).all() and got[1][4].tolist() == [3, 3 + counts[1]]


def test_emit_timed_refuses_bad_arguments():
    dev = _gpu()
    from bmc_hip import lib, slots
    pred = torch.zeros(2, 2, 8, 8, device=dev)
    parts = torch.zeros(8, dtype=torch.int32, device=dev)
    scratch = torch.zeros(slots.emit_timed_scratch_bytes(2, 1, 100), dtype=torch.uint8, device=dev)
    table = slots.SlotTable(2, dev, emit=True, timed=True)
    with pytest.raises(ValueError, match="no timed emit entries"):
        slots.emit_timed(slots.SlotTable(2, dev, emit=True), pred, 255, 1, parts, scratch, 100)
    with pytest.raises(ValueError, match="use emit_timed"):
        slots.emit(table, pred, 255, 1, parts)
    with pytest.raises(ValueError, match="max_count"):
        slots.emit_timed(table, pred, 256, 1, parts, scratch, 100)
    with pytest.raises(ValueError, match="scratch must be"):
        slots.emit_timed(table, pred, 255, 1, parts, scratch, 101)
    with pytest.raises(ValueError, match="window_capacity"):
        slots.emit_timed(table, pred, 255, 1, parts, scratch, 0)
    args = lambda mc, wc: (table.ptr(), table.emit_ptr(), 2, pred.data_ptr(), 8, 8, mc, 1, parts.data_ptr(),
                           slots.emit_rank_table(dev).data_ptr(), scratch.data_ptr(), wc, None)
    with pytest.raises(RuntimeError, match="max_count"):               # ... and the library checks for itself
        lib.call(lib._slot_emit_timed, "bmc_slot_emit_timed", *args(256, 100))
    with pytest.raises(RuntimeError, match="window_capacity"):
        lib.call(lib._slot_emit_timed, "bmc_slot_emit_timed", *args(255, 0))


# ------------------------------------------------------------------ 2. sessions
def _check_timed_stream(res, max_count=255):
    xs, ys, ps = (t.cpu().numpy() for t in res["sr_events"])
    ts = res["sr_ts"].cpu().numpy()
    index = res["sr_index"].numpy()
    preds = res["predictions"].cpu().numpy()
    assert ts.dtype == np.float32 and len(res["sr_events"]) == 3 and len(ts) == len(xs) == index[-1]
    for i, P in enumerate(preds):
        wx, wy, wp, wt, q = emit_timed_np(P, max_count)
        a, b = index[i], index[i + 1]
        assert b - a == len(wx), i
        assert xs[a:b].tobytes() == wx.tobytes() and ys[a:b].tobytes() == wy.tobytes() and ps[a:b].tobytes() == wp.tobytes(), i
        assert ts[a:b].tobytes() == wt.tobytes(), i
        assert (np.diff(ts[a:b]) >= 0).all() and (q > 0).mean() >= 0.05 and q.max() >= 2
    return b"".join(a.tobytes() for a in (xs, ys, ps, ts, index))


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("plain", [False, True])
def test_session_timed_streams_equal_the_restatement(plain, graph):
    """7 recordings of 2-7 windows in 3 slots, frame-backed and event-backed mixed; the whole session twice: identical bytes."""
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(plain, n_c, seed=411).to(dev)
    runs = []
    for _ in range(2):
        ms = MultiStreamSR(m, 3, n_c=n_c, scale=SCALE, plain=plain, graph=graph, keep_predictions=True, emit_events=True,
                           event_times="linear")
        hs = []
        for k, n in enumerate([4, 7, 2, 5, 3, 6, 2]):
            if k % 2:
                lr, gt, li, gi = _event_recording(430 + k, n, H, W)
                hs.append(ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (SCALE * H, SCALE * W)))
                assert ms._recs[hs[-1]]["win_capacity"] == 2 * SCALE ** 2 * int((li[:, 1] - li[:, 0]).max())
            else:
                f, g = _frames(420 + k, n, H, W)
                hs.append(ms.open(f.to(dev), g.to(dev)))
                assert ms._recs[hs[-1]]["win_capacity"] == 2 * SCALE ** 2 * int(f.sum(dim=(1, 2, 3)).max())
        emi, plain_emit = slots.EMIT_TIMED_LAUNCHES, slots.EMIT_LAUNCHES
        ms.run()
        assert slots.EMIT_LAUNCHES == plain_emit and slots.EMIT_TIMED_LAUNCHES > emi
        if graph:
            assert ms._graph is not None and ms.replays > 0
        runs.append(b"".join(_check_timed_stream(ms.results(h)) for h in hs))
        assert ms.scratch_bytes() >= 8 * 3 * ms._wcap
    assert runs[0] == runs[1]


@pytest.mark.parametrize("graph", [False, True])
def test_event_times_off_changes_nothing(graph):
    """event_times=None: the bytes of sr_events / sr_index and every metric equal those of a session that never names the
    option, sr_ts is absent; and with the option on, events (as multisets per window), index and metrics are still the same."""
    dev = _gpu()
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=451).to(dev)
    recs = [_frames(460 + k, n, H, W) for k, n in enumerate([3, 6, 2, 5])]
    out = []
    for kw in ({}, {"event_times": None}, {"event_times": "linear"}):
        ms = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE, graph=graph, emit_events=True, **kw)
        hs = [ms.open(f.to(dev), g.to(dev)) for f, g in recs]
        ms.run()
        out.append([ms.results(h) for h in hs])
        assert ("emit_scratch" in ms._bufs) == (kw.get("event_times") is not None)
        assert ms._bufs["table"].timed == (kw.get("event_times") is not None)
    for a, b, c in zip(*out):
        assert "sr_ts" not in a and "sr_ts" not in b and "sr_ts" in c
        for x in (b, c):
            assert a["esr_mse"] == x["esr_mse"] and a["bicubic_mse"] == x["bicubic_mse"] and torch.equal(a["sr_index"], x["sr_index"])
        assert all(torch.equal(u, v) for u, v in zip(a["sr_events"], b["sr_events"]))
        assert set(a) == set(b)


# ------------------------------------------------------------------ 3. capacities
def test_window_event_capacity_too_small_is_reported_exactly():
    dev = _gpu()
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=491).to(dev)
    recs = [_frames(492 + k, 4, H, W) for k in range(3)]

    def session(wcap1, cap1=None):
        ms = MultiStreamSR(m, 3, n_c=n_c, scale=SCALE, keep_predictions=True, emit_events=True, event_times="linear")
        hs = [ms.open(f.to(dev), g.to(dev), window_event_capacity=wcap1 if k == 1 else None,
                      event_capacity=cap1 if k == 1 else None) for k, (f, g) in enumerate(recs)]
        for h in hs:
            r = ms._recs[h]
            r["ev_xs"].fill_(SENT16), r["ev_ts"].fill_(float(SENTF))
        ms.run()
        return ms, hs

    ms, hs = session(100)
    for k in (0, 2):
        _check_timed_stream(ms.results(hs[k]))
    with pytest.raises(RuntimeError, match=r"window_event_capacity >= (\d+)") as err:
        ms.results(hs[1])
    needed = int(re.search(r"window_event_capacity >= (\d+)", str(err.value)).group(1))
    r = ms._recs[hs[1]]
    per_window = [len(emit_np(P)[0]) for P in r["keep"].cpu().numpy()]
    assert needed == max(per_window) > 100 and int(r["ev_index"][-1]) == sum(per_window)
    ms2, hs2 = session(needed)
    _check_timed_stream(ms2.results(hs2[1]))
    ms3, hs3 = session(needed, cap1=1000)                              # the column capacity, as without times
    with pytest.raises(RuntimeError, match=r"event_capacity >= %d" % sum(per_window)):
        ms3.results(hs3[1])
    r = ms3._recs[hs3[1]]
    want = np.concatenate([emit_timed_np(P)[3] for P in r["keep"].cpu().numpy()])[:1000]
    assert r["ev_ts"].numel() == 1000 and r["ev_ts"].cpu().numpy().tobytes() == want.tobytes()


# ------------------------------------------------------------------ 4. launches
def test_six_kernels_per_window_in_one_call():
    """A window of a timed session makes ONE bmc_slot_emit_timed call (and no bmc_slot_emit call), whatever S; the call is six
    kernel launches (slots.EMIT_TIMED_KERNELS, pinned on the source by test_event_times_cpu)."""
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    assert slots.EMIT_TIMED_KERNELS == 6
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=471).to(dev)
    for S in (1, 4):
        ms = MultiStreamSR(m, S, n_c=n_c, scale=SCALE, emit_events=True, event_times="linear")
        for k in range(S):
            f, g = _frames(472 + k, 3, H, W)
            ms.open(f.to(dev), g.to(dev))
        for _ in range(3):
            before, emi, timed = dict(slots.LAUNCHES), slots.EMIT_LAUNCHES, slots.EMIT_TIMED_LAUNCHES
            assert ms.step()
            assert {k: slots.LAUNCHES[k] - before[k] for k in before} == {"stage": 1, "commit": 1, "metrics": 1}
            assert slots.EMIT_LAUNCHES == emi and slots.EMIT_TIMED_LAUNCHES == timed + 1


# ------------------------------------------------------------------ 5. counts_to_events(times="linear")
@pytest.mark.parametrize("B,sH,sW,max_count", [(1, 36, 56, 255), (5, 124, 224, 255), (3, 37, 53, 2)])
def test_counts_to_events_with_times(B, sH, sW, max_count):
    dev = _gpu()
    from bmc_hip.encodings import counts_to_events
    rng = np.random.default_rng(B * sH + 1)
    preds = np.stack([_synthetic(rng, sH, sW) for _ in range(B)])
    if B > 2:
        preds[1] = 0.0
    plain = counts_to_events(torch.tensor(preds).to(dev), max_count)
    xs, ys, ps, ts, index = counts_to_events(torch.tensor(preds).to(dev), max_count, times="linear")
    assert len(plain) == 4 and torch.equal(plain[3], index) and ts.dtype == torch.float32 and ts.is_cuda
    xs, ys, ps, ts, index = xs.cpu().numpy(), ys.cpu().numpy(), ps.cpu().numpy(), ts.cpu().numpy(), index.numpy()
    for b in range(B):
        wx, wy, wp, wt, _ = emit_timed_np(preds[b], max_count)
        a, z = index[b], index[b + 1]
        assert z - a == len(wx), b
        assert xs[a:z].tobytes() == wx.tobytes() and ys[a:z].tobytes() == wy.tobytes() and ps[a:z].tobytes() == wp.tobytes(), b
        assert ts[a:z].tobytes() == wt.tobytes(), b
    empty = counts_to_events(torch.full((2, 2, 8, 8), -1.0, device=dev), times="linear")
    assert len(empty) == 5 and empty[3].numel() == 0 and empty[4].tolist() == [0, 0, 0]
