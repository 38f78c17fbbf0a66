"""Event output of multi-stream inference on the MI355X (infer.MultiStreamSR(emit_events=True), csrc/slot_emit.hip): the two
emit kernels byte for byte against the numpy restatement (event_output_ref.emit_np), the round trip through the repo's own GPU
encoder, whole sessions against the restatement applied to their kept dense predictions, the reference golden, and that
switching the output on changes nothing else."""
import numpy as np
import pytest
import torch

from event_output_ref import counts_np, emit_np, quantise_np
from test_gpu_r2 import _gpu, load, _restore_math_mode  # noqa: F401
from test_gpu_multistream import SCALE, SEQN, _model
from test_gpu_event_slots import _columns, _dev

pytestmark = pytest.mark.gpu

SENT16, SENT8 = -12345, -77          # what the output columns hold before a run


# ------------------------------------------------------------------ helpers
COMMON = np.array([0.0, -0.0, -0.5, -1.3, 0.3, 0.5, 0.49999997, 1e-30], np.float32)          # all give q = 0
SOME = np.array([0.7, 1.0, 1.5, 2.5, 3.2, 1.49, 0.50000006, 3.5], np.float32)                # q = 1, 1, 2, 2, 3, 1, 1, 4
RARE = np.array([np.nan, np.inf, -np.inf, 300.0, 254.5, 255.5, 7.0, -1e30], np.float32)      # q = 0, max, 0, max, 254, max, 7, 0


def _synthetic(rng, sH, sW):
    """A prediction that meets every branch of the rule: exact ties, negatives, -0.0, NaN, +-inf, values above max_count."""
    kind = rng.random((2, sH, sW))
    P = COMMON[rng.integers(0, len(COMMON), (2, sH, sW))]
    P = np.where(kind > 0.85, SOME[rng.integers(0, len(SOME), (2, sH, sW))], P)
    P = np.where(kind > 0.99, RARE[rng.integers(0, len(RARE), (2, sH, sW))], P)
    return P.astype(np.float32)


def _emit_once(dev, preds, active, entry, base, caps, max_count, nparts=None):
    """One bmc_slot_emit call on predictions preds [S,2,sH,sW] (numpy): slot s is active / has an emit entry as the lists say,
    appends at base[s] into sentinel-filled columns of caps[s] entries -> per slot (xs, ys, ps, index[2]) as numpy."""
    from bmc_hip import slots
    S, _, sH, sW = preds.shape
    nparts = nparts or slots.emit_parts(sH, sW)
    pred = torch.tensor(preds).to(dev)
    cols = [(torch.full((max(c, 1),), SENT16, dtype=torch.int16, device=dev), torch.full((max(c, 1),), SENT16, dtype=torch.int16, device=dev),
             torch.full((max(c, 1),), SENT8, dtype=torch.int8, device=dev)) for c in caps]
    index = torch.tensor([[b, -1] for b in base], dtype=torch.int64).to(dev)
    parts = torch.zeros(S * nparts, dtype=torch.int32, device=dev)
    table = slots.SlotTable(S, dev, emit=True)
    e, em = table.host(), table.emit_host()
    for s in range(S):
        if active[s]:
            e[s]["frames"], e[s]["flags"] = pred.data_ptr(), slots.ACTIVE
        if entry[s]:
            em[s]["xs"], em[s]["ys"], em[s]["ps"] = (t.data_ptr() for t in cols[s])
            em[s]["index_in"], em[s]["index_out"] = index[s].data_ptr(), index[s].data_ptr() + 8
            em[s]["capacity"] = caps[s]
    table.upload()
    before = slots.EMIT_LAUNCHES
    slots.emit(table, pred, max_count, nparts, parts)
    assert slots.EMIT_LAUNCHES == before + 1
    torch.cuda.synchronize()
    return [tuple(t.cpu().numpy() for t in cols[s]) + (index[s].cpu().numpy(),) for s in range(S)]


def _check_slot(got, P, emits, base, cap, max_count):
    """Columns, index and the untouched words around the events of one slot, byte for byte."""
    xs, ys, ps, index = got
    if not emits:
        assert index.tolist() == [base, -1]
        assert (xs == SENT16).all() and (ys == SENT16).all() and (ps == SENT8).all()
        return 0
    wx, wy, wp, q = emit_np(P, max_count)
    n = len(wx)
    assert index.tolist() == [base, base + n]                          # the true running count, also past the capacity
    for g, w, sent in ((xs, wx, SENT16), (ys, wy, SENT16), (ps, wp, SENT8)):
        want = np.full(len(g), sent, g.dtype)
        k = max(0, min(n, cap - base))                                 # events that fit
        want[base:base + k] = w[:k]
        if cap < len(want):
            want[cap:] = sent
        assert g.tobytes() == want.tobytes()
    return n


# ------------------------------------------------------------------ 1. the kernels, byte for byte
@pytest.mark.parametrize("sH,sW,S", [(36, 56, 1), (36, 56, 32), (124, 224, 3), (124, 224, 32), (720, 960, 1), (720, 960, 3),
                                     (37, 53, 3), (37, 53, 32)])
def test_emit_kernels_bit_exact(sH, sW, S):
    """Synthetic predictions with every special value; of the slots, every 5th + 1 is inactive, every 5th + 3 has no emit entry,
    slot 2 (where there is one) is all zero, one slot's capacity ends in the middle of its events; the streams start at odd
    positions inside sentinel-filled columns.  37x53 takes the unaligned (scalar-load) path: 2*37*53 is no multiple of 4."""
    dev = _gpu()
    rng = np.random.default_rng(1000 * sH + S)
    preds = np.stack([_synthetic(rng, sH, sW) for _ in range(S)])
    if S > 2:
        preds[2] = np.where(preds[2] > 0, -preds[2], preds[2])         # nothing positive: zero events
        preds[2][np.isnan(preds[2])] = 0.0
    active = [s % 5 != 1 for s in range(S)]
    entry = [s % 5 != 3 for s in range(S)]
    counts = [int(quantise_np(p).sum()) for p in preds]
    base = [0 if s == 0 else 3 + 7 * s for s in range(S)]
    caps = [base[s] + counts[s] + 50 for s in range(S)]
    cut = S - 1 if S > 1 else None                                     # (S-1) % 5 is 2 at S = 3 -> use slot 0 there
    if cut is not None and (not active[cut] or not entry[cut] or counts[cut] < 10):
        cut = 0
    if cut is not None:
        caps[cut] = base[cut] + counts[cut] // 2 + 1
    runs = []
    for _ in range(2):
        got = _emit_once(dev, preds, active, entry, base, caps, 255)
        total = 0
        for s in range(S):
            total += _check_slot(got[s], preds[s], active[s] and entry[s], base[s], caps[s], 255)
        assert total > 0.2 * preds[0].size
        runs.append(b"".join(a.tobytes() for g in got for a in g))
    assert runs[0] == runs[1]
    if S > 2:
        assert got[2][3].tolist() == [base[2], base[2]]                # the all-zero prediction: index[i+1] == index[i]


@pytest.mark.parametrize("sH,sW,max_count,value", [(36, 56, 255, 1000.0), (36, 56, 1, 0.7), (124, 224, 3, np.inf), (8, 8, 32767, 1e9),
                                                   (720, 960, 2, 2.5)])
def test_all_max_count(sH, sW, max_count, value):
    """Every element at max_count: the densest stream there is (tile totals far above the workgroup size)."""
    dev = _gpu()
    P = np.full((1, 2, sH, sW), value, np.float32)
    n = 2 * sH * sW * max_count
    (got,) = _emit_once(dev, P, [True], [True], [5], [5 + n + 9], max_count)
    assert _check_slot(got, P[0], True, 5, 5 + n + 9, max_count) == n


@pytest.mark.parametrize("nparts", [1, 2, 7, 64, 1024])
def test_any_number_of_parts_gives_the_same_stream(nparts):
    """The split into parts is an implementation detail: parts that own nothing (more parts than 4-element groups) included."""
    dev = _gpu()
    rng = np.random.default_rng(nparts)
    preds = np.stack([_synthetic(rng, 36, 56) for _ in range(3)])
    counts = [int(quantise_np(p).sum()) for p in preds]
    got = _emit_once(dev, preds, [True] * 3, [True] * 3, [0, 11, 0], [c + 20 for c in counts], 255, nparts=nparts)
    for s in range(3):
        _check_slot(got[s], preds[s], True, [0, 11, 0][s], counts[s] + 20, 255)


def _with_silent_waves(P, parts):
    """P with whole waves of a scan tile silenced.  A tile is 1 024 consecutive elements, 256 per wave, and with `parts` parts of
    2 048 elements the tiles start at multiples of 1 024: wave 1 of tile 0, wave 0 of tile 2 and wave 3 of tile 3 emit nothing,
    and neither does the whole last part."""
    flat = P.copy().reshape(-1)
    assert flat.size == 2048 * parts and parts >= 3
    for lo in (256, 2048, 3 * 1024 + 768):
        flat[lo:lo + 256] = -1.0
    flat[2048 * (parts - 1):] = -1.0
    return flat.reshape(P.shape)


def test_a_wave_and_a_part_without_events():
    """Zero wave totals in the tile scan and a zero part total in the sum of the parts before a part."""
    dev = _gpu()
    rng = np.random.default_rng(64)
    sH, sW, parts = 32, 96, 3                                          # 6 144 elements: three parts of two tiles
    P = _synthetic(rng, sH, sW)
    P = _with_silent_waves(np.where(quantise_np(P) > 0, P, np.float32(1.0)), parts)       # every other element emits
    q = quantise_np(P).reshape(-1)
    assert q[256:512].sum() == 0 and q[2048:2304].sum() == 0 and q[4096:].sum() == 0 and (q[:256] > 0).all()
    n = int(q.sum())
    (got,) = _emit_once(dev, P[None], [True], [True], [3], [3 + n + 9], 255, nparts=parts)
    assert _check_slot(got, P, True, 3, 3 + n + 9, 255) == n


def test_emit_refuses_bad_arguments():
    dev = _gpu()
    from bmc_hip import slots
    pred = torch.zeros(2, 2, 8, 8, device=dev)
    parts = torch.zeros(8, dtype=torch.int32, device=dev)
    table = slots.SlotTable(2, dev, emit=True)
    with pytest.raises(ValueError, match="no emit entries"):
        slots.emit(slots.SlotTable(2, dev, events=True), pred, 255, 1, parts)
    with pytest.raises(ValueError, match="parts must be"):
        slots.emit(table, pred, 255, 8, parts)                         # 2 x 8 words needed
    with pytest.raises(ValueError, match="parts must be"):
        slots.emit(table, pred, 255, 1, parts.float())
    with pytest.raises(ValueError, match="pred must be"):
        slots.emit(table, pred[:1], 255, 1, parts)
    with pytest.raises(ValueError, match="overflow"):
        slots.emit(table, torch.zeros(2, 2, 512, 512, device=dev), 32767, 1, parts)
    from bmc_hip import lib                                            # ... and the library checks for itself
    with pytest.raises(RuntimeError, match="nparts"):
        lib.call(lib._slot_emit, "bmc_slot_emit", table.ptr(), table.emit_ptr(), 2, pred.data_ptr(), 8, 8, 255, 1025,
                 parts.data_ptr(), None)
    with pytest.raises(RuntimeError, match="max_count"):
        lib.call(lib._slot_emit, "bmc_slot_emit", table.ptr(), table.emit_ptr(), 2, pred.data_ptr(), 8, 8, 0, 1,
                 parts.data_ptr(), None)
    with pytest.raises(RuntimeError, match="int16"):
        lib.call(lib._slot_emit, "bmc_slot_emit", table.ptr(), table.emit_ptr(), 2, pred.data_ptr(), 8, 32768, 255, 1,
                 parts.data_ptr(), None)


# ------------------------------------------------------------------ 2. round trip through the repo's GPU encoder
@pytest.mark.parametrize("sH,sW,S", [(36, 56, 3), (124, 224, 3), (720, 960, 1)])
def test_round_trip_through_the_gpu_encoder(sH, sW, S):
    dev = _gpu()
    from bmc_hip import ops
    rng = np.random.default_rng(sH + S)
    preds = np.stack([_synthetic(rng, sH, sW) for _ in range(S)])
    counts = [int(quantise_np(p).sum()) for p in preds]
    got = _emit_once(dev, preds, [True] * S, [True] * S, [0] * S, counts, 255)
    for s in range(S):
        xs, ys, ps, index = got[s]
        assert index.tolist() == [0, counts[s]] and len(xs) == counts[s]
        off = torch.tensor([0, counts[s]], dtype=torch.int64, device=dev)
        img = ops.encode_raw_events(torch.tensor(xs).to(dev), torch.tensor(ys).to(dev), torch.tensor(ps.astype(np.float64)).to(dev),
                                    off, None, sH, sW)
        assert np.array_equal(img[0].cpu().numpy(), quantise_np(preds[s]).astype(np.float32)), s


# ------------------------------------------------------------------ 3. sessions
def _frames(seed, n_windows, H, W, mean=1.0):
    g = torch.Generator().manual_seed(seed)
    L = n_windows + SEQN - 1
    return (torch.poisson(torch.full((L, 2, H, W), mean), generator=g),
            torch.poisson(torch.full((L, 2, SCALE * H, SCALE * W), 0.1), generator=g))


def _event_recording(seed, n_windows, H, W):
    """A synthetic event recording with about one LR event per element of a frame."""
    from bmc_hip.encodings import event_window_indices
    rng = np.random.default_rng(seed)
    window = 2 * H * W
    L = n_windows + SEQN - 1
    n_lr = (window // 2) * L + 7
    n_gt = SCALE * SCALE * n_lr
    lr, gt = _columns(rng, n_lr, H, W), _columns(rng, n_gt, SCALE * H, SCALE * W)
    lr_index, gt_index = event_window_indices(np.sort(rng.uniform(0, 1, n_lr)), np.sort(rng.uniform(0, 1, n_gt)), window,
                                              window // 2, SCALE)
    assert len(lr_index) == L
    return lr, gt, lr_index, gt_index


def _check_stream(res, sH, sW, max_count=255):
    """Every window's events == the restatement applied to the kept dense prediction of that window, and the stream is a real
    one: events on at least 5 % of the elements, a count >= 2, both polarities -- in EVERY window."""
    xs, ys, ps = (t.cpu().numpy() for t in res["sr_events"])
    index = res["sr_index"].numpy()
    preds = res["predictions"].cpu().numpy()
    assert xs.dtype == np.int16 and ys.dtype == np.int16 and ps.dtype == np.int8 and index.dtype == np.int64
    assert len(index) == len(preds) + 1 and index[0] == 0 and len(xs) == len(ys) == len(ps) == index[-1]
    for i, P in enumerate(preds):
        wx, wy, wp, q = emit_np(P, max_count)
        a, b = index[i], index[i + 1]
        assert b - a == len(wx), i
        assert xs[a:b].tobytes() == wx.tobytes() and ys[a:b].tobytes() == wy.tobytes() and ps[a:b].tobytes() == wp.tobytes(), i
        assert (q > 0).mean() >= 0.05 and q.max() >= 2 and (wp > 0).any() and (wp < 0).any(), (i, (q > 0).mean(), q.max())
        assert np.array_equal(counts_np(xs[a:b], ys[a:b], ps[a:b], sH, sW), q)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("plain", [False, True])
def test_session_streams_equal_the_restatement_of_the_kept_predictions(plain, graph):
    """7 recordings of 2-7 windows in 3 slots, frame-backed and event-backed mixed: recordings join and leave mid-run."""
    dev = _gpu()
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(plain, n_c, seed=211).to(dev)
    ms = MultiStreamSR(m, 3, n_c=n_c, scale=SCALE, plain=plain, graph=graph, keep_predictions=True, emit_events=True)
    hs = []
    for k, n in enumerate([4, 7, 2, 5, 3, 6, 2]):
        if k % 2:
            lr, gt, li, gi = _event_recording(230 + k, n, H, W)
            hs.append((n, ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (SCALE * H, SCALE * W))))
        else:
            f, g = _frames(220 + k, n, H, W)
            hs.append((n, ms.open(f.to(dev), g.to(dev))))
    ms.run()
    if graph:
        assert ms._graph is not None and ms.replays > 0
    for n, h in hs:
        res = ms.results(h)
        assert len(res["esr_mse"]) == n == len(res["sr_index"]) - 1
        _check_stream(res, SCALE * H, SCALE * W)


def test_session_max_count_and_partial_results():
    """max_count = 1 clamps every count; results() before the end gives the windows done so far."""
    dev = _gpu()
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=241).to(dev)
    ms = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE, keep_predictions=True, emit_events=True, max_count=1)
    f, g = _frames(242, 5, H, W)
    h = ms.open(f.to(dev), g.to(dev))
    for done in (1, 2, 3):
        assert ms.step()
        res = ms.results(h)
        assert len(res["sr_index"]) == done + 1 and res["predictions"].shape[0] == done
        xs, ys, ps = (t.cpu().numpy() for t in res["sr_events"])
        idx = res["sr_index"].numpy()
        for i in range(done):
            wx, wy, wp, q = emit_np(res["predictions"][i].cpu().numpy(), 1)
            assert q.max() == 1 and idx[i + 1] - idx[i] == q.sum() > 0.05 * q.size
            assert xs[idx[i]:idx[i + 1]].tobytes() == wx.tobytes() and ps[idx[i]:idx[i + 1]].tobytes() == wp.tobytes()


# ------------------------------------------------------------------ 4. the reference golden
@pytest.mark.parametrize("graph", [False, True])
def test_reference_golden_as_event_stream(graph):
    """infer_seqn3.npz through evaluate_recordings(emit_events=True): the count image rebuilt from the emitted events equals
    rint / clamp of the reference's own predictions, except where the golden value lies within 1e-4 (parity_bars.CONTRACT_SR) of
    a half-integer: there they may differ by exactly 1.  5 of the golden's 32 256 elements are that close to a tie."""
    dev = _gpu()
    from infer import evaluate_recordings
    from models.BMCNet import BMCNet
    from parity_bars import CONTRACT_SR
    from test_gpu_parity import _load_sd
    z = load("infer_seqn3.npz")
    scale, n_c, n_b, B, H, W, seqn, nwin, gh, gw = (int(v) for v in z["meta"])
    m = BMCNet(scale, n_c, n_b)
    _load_sd(m, z)
    m.to(dev)
    frames, gts = torch.tensor(z["frames"]).to(dev), torch.tensor(z["gts"]).to(dev)
    recs = {"sample%d" % b: (frames[b, :nwin + seqn - 1], gts[b, :nwin + seqn - 1]) for b in range(B)}
    out = evaluate_recordings(m, recs, 2, n_c=n_c, scale=scale, graph=graph, seqn=seqn, gt_size=(gh, gw), emit_events=True)
    assert CONTRACT_SR == 1e-4 and "predictions" not in out
    near, differ = 0, 0
    for b in range(B):
        xs, ys, ps, index = out["sr_events"]["sample%d" % b]
        xs, ys, ps, index = xs.cpu().numpy(), ys.cpu().numpy(), ps.cpu().numpy(), index.numpy()
        assert len(index) == nwin + 1 and index[0] == 0 and index[-1] == len(xs)
        for i in range(nwin):
            G = z["pred%d" % i][b]
            want = quantise_np(G)
            got = counts_np(xs[index[i]:index[i + 1]], ys[index[i]:index[i + 1]], ps[index[i]:index[i + 1]], scale * H, scale * W)
            tie = np.abs(G.astype(np.float64) - np.floor(G.astype(np.float64)) - 0.5) <= CONTRACT_SR
            near += int(tie.sum())
            d = np.abs(got - want)
            differ += int((d != 0).sum())
            print("golden window", b, i, "events", index[i + 1] - index[i], "near ties", int(tie.sum()), "differing", int((d != 0).sum()))
            assert (d[~tie] == 0).all(), (b, i)
            assert (d[tie] <= 1).all(), (b, i)
            assert index[i + 1] - index[i] >= 2000 and want.max() >= 2
    assert near <= 5 and differ <= near


# ------------------------------------------------------------------ 5. emission changes nothing else
@pytest.mark.parametrize("graph", [False, True])
def test_emission_changes_nothing_else(graph):
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=251).to(dev)
    recs = [_frames(260 + k, n, H, W) for k, n in enumerate([3, 6, 2, 5])]
    out = {}
    for emit in (False, True):
        ms = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE, graph=graph, keep_predictions=True, emit_events=emit)
        hs = [ms.open(f.to(dev), g.to(dev)) for f, g in recs]
        launches = []
        while True:
            before, enc, emi = dict(slots.LAUNCHES), slots.ENCODE_LAUNCHES, slots.EMIT_LAUNCHES
            if not ms.step():
                break
            launches.append(({k: slots.LAUNCHES[k] - before[k] for k in before}, slots.ENCODE_LAUNCHES - enc,
                             slots.EMIT_LAUNCHES - emi))
        torch.cuda.synchronize()
        out[emit] = ([ms.results(h) for h in hs], ms._bufs["pool"].clone(), ms._bufs["pred"].clone(), launches, ms.replays)
        assert ("emit_parts" in ms._bufs) == emit and ms._bufs["table"].emit == emit
    (ra, pool_a, pred_a, la, rep_a), (rb, pool_b, pred_b, lb, rep_b) = out[False], out[True]
    for a, b in zip(ra, rb):
        assert a["esr_mse"] == b["esr_mse"] and a["bicubic_mse"] == b["bicubic_mse"]
        assert torch.equal(a["predictions"], b["predictions"])
        assert "sr_events" not in a and "sr_index" not in a and "sr_events" in b
    assert torch.equal(pool_a, pool_b) and torch.equal(pred_a, pred_b) and rep_a == rep_b
    one = {"stage": 1, "commit": 1, "metrics": 1}
    none = {"stage": 0, "commit": 0, "metrics": 0}
    assert len(la) == len(lb) >= 8
    for k, (x, y) in enumerate(zip(la, lb)):
        eager = not graph or k < 2 or k == 2                           # the third window captures (wrappers run once) and replays
        assert x == ((one if eager else none), 0, 0), (k, x)           # off: no emit launch, ever
        assert y == ((one if eager else none), 0, 1 if eager else 0), (k, y)     # on: exactly one emit call per window


@pytest.mark.parametrize("S", [1, 4])
def test_one_emit_call_per_window_whatever_S(S):
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=271).to(dev)
    ms = MultiStreamSR(m, S, n_c=n_c, scale=SCALE, emit_events=True)
    for k in range(S):
        f, g = _frames(272 + k, 3, H, W)
        ms.open(f.to(dev), g.to(dev))
    for _ in range(3):
        before, emi = dict(slots.LAUNCHES), slots.EMIT_LAUNCHES
        assert ms.step()
        assert {k: slots.LAUNCHES[k] - before[k] for k in before} == {"stage": 1, "commit": 1, "metrics": 1}
        assert slots.EMIT_LAUNCHES == emi + 1
    assert set(slots.LAUNCHES) == {"stage", "commit", "metrics"}


def test_late_event_backed_recording_keeps_the_emit_table():
    """A frames-only emitting session that gets its first event-backed recording after the capture: the table is rebuilt with
    both the event and the emit part, and the streams go on where they were."""
    dev = _gpu()
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=281).to(dev)
    ms = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE, graph=True, keep_predictions=True, emit_events=True)
    f, g = _frames(282, 8, H, W)
    h0 = ms.open(f.to(dev), g.to(dev))
    for _ in range(4):
        ms.step()
    assert ms._graph is not None
    lr, gt, li, gi = _event_recording(283, 4, H, W)
    h1 = ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (SCALE * H, SCALE * W))
    assert ms._graph is None and ms._bufs["table"].events and ms._bufs["table"].emit
    ms.run()
    for h in (h0, h1):
        _check_stream(ms.results(h), SCALE * H, SCALE * W)


# ------------------------------------------------------------------ 6. capacity
def test_capacity_too_small_is_reported_exactly():
    dev = _gpu()
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    sH, sW = SCALE * H, SCALE * W
    m = _model(False, n_c, seed=291).to(dev)
    recs = [_frames(292 + k, 4, H, W) for k in range(3)]

    def session(cap1):
        ms = MultiStreamSR(m, 3, n_c=n_c, scale=SCALE, keep_predictions=True, emit_events=True)
        hs = [ms.open(f.to(dev), g.to(dev), event_capacity=cap1 if k == 1 else None) for k, (f, g) in enumerate(recs)]
        for h in hs:                                                   # sentinels behind whatever gets written
            r = ms._recs[h]
            r["ev_xs"].fill_(SENT16), r["ev_ys"].fill_(SENT16), r["ev_ps"].fill_(SENT8)
        ms.run()
        return ms, hs

    ms, hs = session(1000)
    for k in (0, 2):                                                   # the neighbours' streams are whole
        _check_stream(ms.results(hs[k]), sH, sW)
        r = ms._recs[hs[k]]
        assert r["ev_capacity"] == 2 * SCALE ** 2 * int(recs[k][0].sum().item())      # the default: 2 x scale^2 x LR events
        total = int(r["ev_index"][-1])
        assert total <= r["ev_capacity"] and (r["ev_xs"][total:] == SENT16).all() and (r["ev_ps"][total:] == SENT8).all()
    with pytest.raises(RuntimeError, match=r"event_capacity >= (\d+)") as err:
        ms.results(hs[1])
    import re
    needed = int(re.search(r"event_capacity >= (\d+)", str(err.value)).group(1))
    r = ms._recs[hs[1]]
    full = [emit_np(P)[0] for P in r["keep"].cpu().numpy()]
    assert needed == sum(len(x) for x in full) > 1000 and int(r["ev_index"][-1]) == needed
    assert r["ev_xs"].numel() == 1000                                  # the columns end at the capacity: nothing lies behind it
    assert r["ev_xs"].cpu().numpy().tobytes() == np.concatenate(full)[:1000].astype(np.int16).tobytes()
    ms2, hs2 = session(needed)
    res = ms2.results(hs2[1])
    _check_stream(res, sH, sW)
    assert int(res["sr_index"][-1]) == needed == res["sr_events"][0].numel()


def test_words_behind_a_small_capacity_keep_their_sentinel():
    """The kernel honours `capacity`, not the allocation: columns longer than the capacity keep their sentinel behind it."""
    dev = _gpu()
    rng = np.random.default_rng(301)
    preds = np.stack([_synthetic(rng, 36, 56) for _ in range(2)])
    counts = [int(quantise_np(p).sum()) for p in preds]
    from bmc_hip import slots
    S, nparts = 2, slots.emit_parts(36, 56)
    pred = torch.tensor(preds).to(dev)
    cols = [[torch.full((counts[s] + 64,), SENT16 if k < 2 else SENT8, dtype=torch.int16 if k < 2 else torch.int8, device=dev)
             for k in range(3)] for s in range(S)]
    index = torch.tensor([[0, -1], [0, -1]], dtype=torch.int64).to(dev)
    caps = [100, counts[1]]
    table = slots.SlotTable(S, dev, emit=True)
    e, em = table.host(), table.emit_host()
    for s in range(S):
        e[s]["frames"], e[s]["flags"] = pred.data_ptr(), slots.ACTIVE
        em[s]["xs"], em[s]["ys"], em[s]["ps"] = (t.data_ptr() for t in cols[s])
        em[s]["index_in"], em[s]["index_out"], em[s]["capacity"] = index[s].data_ptr(), index[s].data_ptr() + 8, caps[s]
    table.upload()
    slots.emit(table, pred, 255, nparts, torch.zeros(S * nparts, dtype=torch.int32, device=dev))
    for s in range(S):
        wx, wy, wp, _ = emit_np(preds[s])
        assert index[s].tolist() == [0, counts[s]]
        for t, w, sent in zip(cols[s], (wx, wy, wp), (SENT16, SENT16, SENT8)):
            got = t.cpu().numpy()
            assert got[:caps[s]].tobytes() == w[:caps[s]].tobytes() and (got[caps[s]:] == sent).all(), s


@pytest.mark.parametrize("keep", [False, True])
def test_resident_bytes_events_against_dense(keep):
    """What the sizes imply: 5 bytes per event of capacity + 8 per index entry, against 8 * sH * sW bytes per window."""
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    n_c, H, W, nwin = 16, 10, 16, 5
    sH, sW = SCALE * H, SCALE * W
    m = _model(False, n_c, seed=311).to(dev)
    f, g = _frames(312, nwin, H, W)
    lr, gt, li, gi = _event_recording(313, nwin, H, W)
    L = nwin + SEQN - 1
    sums = nwin * slots.metric_parts(sH, sW) * 2 * 8
    dense = nwin * 2 * sH * sW * 4 if keep else 0
    ms = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE, keep_predictions=keep, emit_events=True)
    hf = ms.open(f.to(dev), g.to(dev))
    he = ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (sH, sW))
    hc = ms.open(f.to(dev), g.to(dev), event_capacity=777)
    cap_f = 2 * SCALE ** 2 * int(f.sum().item())
    cap_e = 2 * SCALE ** 2 * int((li[:, 1] - li[:, 0]).sum())
    stream = lambda cap: 5 * cap + 8 * (nwin + 1)
    assert ms.resident_bytes(hf) == 4 * 2 * L * (H * W + sH * sW) + sums + dense + stream(cap_f)
    assert ms.resident_bytes(he) == 12 * (len(lr[0]) + len(gt[0])) + sums + dense + stream(cap_e)
    assert ms.resident_bytes(hc) == 4 * 2 * L * (H * W + sH * sW) + sums + dense + stream(777)
    off = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE, keep_predictions=True)
    ho = off.open(f.to(dev), g.to(dev))
    assert off.resident_bytes(ho) == 4 * 2 * L * (H * W + sH * sW) + sums + nwin * 2 * sH * sW * 4
    # the ratio of the two outputs for this recording, from the sizes alone
    assert (nwin * 8 * sH * sW) / stream(777) == pytest.approx(102400 / 3933)


# ------------------------------------------------------------------ 7. counts_to_events on a plain tensor
@pytest.mark.parametrize("B,sH,sW,max_count", [(1, 36, 56, 255), (5, 124, 224, 255), (3, 37, 53, 2), (2, 720, 960, 255)])
def test_counts_to_events(B, sH, sW, max_count):
    dev = _gpu()
    from bmc_hip.encodings import counts_to_events
    rng = np.random.default_rng(B * sH)
    preds = np.stack([_synthetic(rng, sH, sW) for _ in range(B)])
    if B > 2:
        preds[1] = 0.0
    xs, ys, ps, index = counts_to_events(torch.tensor(preds).to(dev), max_count)
    assert xs.dtype == torch.int16 and ys.dtype == torch.int16 and ps.dtype == torch.int8 and index.dtype == torch.int64
    assert not index.is_cuda and index[0] == 0 and len(index) == B + 1 and index[-1] == xs.numel() == ys.numel() == ps.numel()
    xs, ys, ps, index = xs.cpu().numpy(), ys.cpu().numpy(), ps.cpu().numpy(), index.numpy()
    for b in range(B):
        wx, wy, wp, _ = emit_np(preds[b], max_count)
        a, z = index[b], index[b + 1]
        assert z - a == len(wx), b
        assert xs[a:z].tobytes() == wx.tobytes() and ys[a:z].tobytes() == wy.tobytes() and ps[a:z].tobytes() == wp.tobytes(), b


def test_counts_to_events_of_nothing():
    dev = _gpu()
    from bmc_hip.encodings import counts_to_events
    xs, ys, ps, index = counts_to_events(torch.full((2, 2, 8, 8), -1.0, device=dev))
    assert xs.numel() == ys.numel() == ps.numel() == 0 and index.tolist() == [0, 0, 0]


def test_counts_to_events_non_contiguous_and_streaming_output():
    """What a StreamingSR user has: the prediction tensor of a step, possibly a view."""
    dev = _gpu()
    from bmc_hip.encodings import counts_to_events
    rng = np.random.default_rng(7)
    big = np.stack([_synthetic(rng, 36, 112) for _ in range(2)])
    view = torch.tensor(big).to(dev)[:, :, :, ::2]
    xs, ys, ps, index = counts_to_events(view)
    for b in range(2):
        wx, wy, wp, _ = emit_np(big[b][:, :, ::2])
        a, z = int(index[b]), int(index[b + 1])
        assert xs[a:z].cpu().numpy().tobytes() == wx.tobytes() and ps[a:z].cpu().numpy().tobytes() == wp.tobytes()
