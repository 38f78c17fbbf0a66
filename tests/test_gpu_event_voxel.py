"""Per-window voxel grids on the GPU (include/bmc_hip.h, "voxel grids"): bmc_slot_voxel through the plain-tensor entry against
the grids the reference's events_to_voxel_torch returned, against the numpy restatement (tests/event_voxel_ref.py) and against
the composition it replaces on the GPU (timed stream -> encodings.events_to_voxel_torch), and MultiStreamSR(voxel_bins=...)
against the restatement of the predictions the session itself exposes -- all byte for byte."""
import functools

import numpy as np
import pytest
import torch

import event_voxel_ref as V
from event_output_ref import quantise_np
from test_event_voxel_cpu import golden_cases
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_multistream import SCALE, SEQN, _model, _recordings

pytestmark = pytest.mark.gpu
N_C = 16
BINS = 5
ALL_BINS = (1, 2, 5, 32)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ (a) the plain-tensor entry
def test_counts_to_voxel_equals_the_reference_and_the_restatement():
    dev = _gpu()
    from bmc_hip.encodings import counts_to_voxel
    n = 0
    for name, q, bins, vox in golden_cases():
        P = q.astype(np.float32)
        out = counts_to_voxel(torch.tensor(P)[None].to(dev), bins)
        assert out.dtype == torch.float32 and tuple(out.shape) == (1,) + vox.shape
        assert _np(out[0]).tobytes() == vox.tobytes(), name
        assert _np(out[0]).tobytes() == V.voxel_np(P, bins).tobytes(), name
        n += 1
    assert n == 19


def _oracle(pred, bins, max_count=255):
    """The composition on the GPU: the timed stream of every image (bmc_slot_emit_timed), its columns as float32 through the
    project's events_to_voxel_torch (csrc/scatter.hip) -> [B,bins,sH,sW]."""
    from bmc_hip import encodings
    B, _, sH, sW = pred.shape
    xs, ys, ps, ts, index = encodings.counts_to_events(pred, max_count, times="linear")
    assert ts.dtype == torch.float32
    out = []
    for b in range(B):
        lo, hi = int(index[b]), int(index[b + 1])
        out.append(encodings.events_to_voxel_torch(xs[lo:hi].float(), ys[lo:hi].float(), ts[lo:hi].clone(), ps[lo:hi].float(), bins,
                                                   sensor_size=(sH, sW)))
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def _image(kind):
    """The prediction of a case (float32 numpy [B,2,sH,sW])."""
    if kind == "ties":                                     # 9 x 12, small counts: 1/2 = 2/4, every j = 0, every j = n-1
        rng = np.random.default_rng(912)
        return rng.choice([0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 5, 7, 9], (1, 2, 9, 12)).astype(np.float32)
    if kind == "large":                                    # 7 x 9, counts 31 .. 255 among small ones, 300 clamped to 255
        rng = np.random.default_rng(79)
        P = rng.choice([0, 0, 0, 0, 1, 2, 3, 5], (1, 2, 7, 9)).astype(np.float32)
        for k, v in enumerate([31, 47, 64, 101, 255, 33, 128, 300, 254]):
            P[0, k % 2, (3 * k) % 7, (5 * k + 1) % 9] = v
        return P
    if kind == "odd":                                      # 5 x 7: 2 * 35 elements, no vector loads; fractions, negatives, a NaN
        rng = np.random.default_rng(57)
        P = (rng.poisson(1.2, (1, 2, 5, 7)) + rng.uniform(-0.5, 0.5, (1, 2, 5, 7))).astype(np.float32)
        P[0, 0, 2, 3], P[0, 1, 4, 6], P[0, 1, 0, 0] = np.nan, -2.0, 2.5
        return P
    if kind == "parts":                                    # 70 x 130: 5 parts in both launches
        rng = np.random.default_rng(70130)
        P = (rng.poisson(0.3, (1, 2, 70, 130)) * rng.uniform(0.6, 1.4, (1, 2, 70, 130))).astype(np.float32)
        P[0, 0, 69, 129], P[0, 1, 69, 129], P[0, 1, 0, 0], P[0, 0, 35, 1] = 17.0, 12.0, 40.0, 255.5
        return P
    raise KeyError(kind)


def test_the_cases_are_what_they_claim():
    from bmc_hip import slots
    assert quantise_np(_image("large")[0]).max() == 255 and (_image("large") == 300).any()
    assert sorted(set(quantise_np(_image("large")[0]).ravel()) & {31, 33, 47, 64, 101, 128, 254, 255}) == [31, 33, 47, 64, 101, 128, 254, 255]
    assert _image("odd").shape[-1] % 2 == 1 and (2 * 5 * 7) % 4 != 0 and np.isnan(_image("odd")).any()
    assert slots.voxel_parts(70, 130) == 5 >= 3 and slots.voxel_parts(36, 48) == 1 and (70 * 130) % 5 == 0 and (2 * 70 * 130) % 4096 != 0
    assert slots.voxel_parts(69, 129) == 5 and (69 * 129) % 5 != 0


@pytest.mark.parametrize("bins", ALL_BINS)
@pytest.mark.parametrize("kind", ["ties", "large", "odd", "parts"])
def test_counts_to_voxel_equals_the_composition_on_the_gpu(kind, bins):
    dev = _gpu()
    from bmc_hip import slots
    from bmc_hip.encodings import counts_to_voxel
    P = _image(kind)
    pred = torch.tensor(P).to(dev)
    before = slots.VOXEL_LAUNCHES
    got = counts_to_voxel(pred, bins)
    assert slots.VOXEL_LAUNCHES == before + 1              # one call = two launches for the whole batch
    want = _oracle(pred, bins)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert _np(got).tobytes() == _np(want).tobytes()
    assert _np(got).tobytes() == np.stack([V.voxel_np(p, bins) for p in P]).tobytes()
    assert got.any()
    assert torch.equal(got, counts_to_voxel(pred, bins))  # the same bytes run after run


def test_counts_to_voxel_ragged_pixel_parts_and_max_count():
    """69 x 129: the voxel launch's last part is shorter than the others; max_count = 7 clamps what the grid sees."""
    dev = _gpu()
    from bmc_hip.encodings import counts_to_voxel
    P = np.ascontiguousarray(_image("parts")[:, :, 1:, 1:])
    pred = torch.tensor(P).to(dev)
    for max_count in (255, 7):
        got = counts_to_voxel(pred, BINS, max_count=max_count)
        assert _np(got).tobytes() == _np(_oracle(pred, BINS, max_count)).tobytes()
        assert _np(got[0]).tobytes() == V.voxel_np(P[0], BINS, max_count).tobytes()


def test_counts_to_voxel_more_than_one_table_group():
    """MAX_SLOTS + 1 images: two slot tables; image 256 is alone in the second.  Some images have 3 events or fewer."""
    dev = _gpu()
    from bmc_hip import slots
    from bmc_hip.encodings import counts_to_voxel
    rng = np.random.default_rng(257)
    B = slots.MAX_SLOTS + 1
    P = rng.choice([0, 0, 0, 0, 1, 1, 2, 3, 6], (B, 2, 4, 6)).astype(np.float32)
    P[3] = 0
    P[7] = 0
    P[7, 0, 1, 1], P[7, 1, 2, 2] = 2, 1                    # N = 3
    P[B - 1, 0, 3, 5] = 11
    pred = torch.tensor(P).to(dev)
    before = slots.VOXEL_LAUNCHES
    got = counts_to_voxel(pred, 2)
    assert slots.VOXEL_LAUNCHES == before + 2
    assert _np(got).tobytes() == _np(_oracle(pred, 2)).tobytes()
    assert _np(got).tobytes() == np.stack([V.voxel_np(p, 2) for p in P]).tobytes()
    assert not got[3].any() and not got[7].any() and got[B - 1].any() and got[0].any()


# ------------------------------------------------------------------ (b) the slot call
@pytest.mark.parametrize("sH,sW", [(5, 7), (70, 130)])
def test_slot_voxel_touches_only_its_slots(sH, sW):
    """Slots 0 and 1 active with a grid, slot 2 inactive with every pointer set, slot 3 active without a dst, slot 4 active with a
    dst but without a prediction: the last three are untouched, and so is every guard."""
    dev = _gpu()
    from bmc_hip import slots
    rng = np.random.default_rng(sH * sW)
    S, n, guard = 5, BINS * sH * sW, 64
    P = rng.poisson(0.8, (S, 2, sH, sW)).astype(np.float32)
    pred = torch.tensor(P).to(dev)
    stride = n + 2 * guard
    buf = torch.full((S * stride,), 77.0, device=dev)
    off = [s * stride + guard for s in range(S)]
    table = slots.SlotTable(S, dev, voxel=True)
    e = table.host()
    vx = table.voxel_host()
    for s in range(S):
        e[s]["frames"], e[s]["flags"] = 0 if s == 4 else pred[s].data_ptr(), 0 if s == 2 else slots.ACTIVE
        vx[s]["dst"] = 0 if s == 3 else buf.data_ptr() + 4 * off[s]
    table.upload()
    nparts = slots.voxel_parts(sH, sW)
    parts = torch.zeros(2 * S * nparts, dtype=torch.int32, device=dev)
    before = slots.VOXEL_LAUNCHES
    slots.voxel(table, pred, 255, BINS, nparts, parts)
    torch.cuda.synchronize()
    assert slots.VOXEL_LAUNCHES == before + 1
    keep = torch.ones_like(buf, dtype=torch.bool)
    for s in (0, 1):
        assert _np(buf[off[s]:off[s] + n]).tobytes() == V.voxel_np(P[s], BINS).tobytes(), s
        keep[off[s]:off[s] + n] = False
    assert (buf[keep] == 77).all()
    first = buf.clone()
    slots.voxel(table, pred, 255, BINS, nparts, parts)                         # the same bytes run after run
    torch.cuda.synchronize()
    assert torch.equal(first, buf)
    with pytest.raises(ValueError, match="no voxel entries"):
        slots.voxel(slots.SlotTable(S, dev), pred, 255, BINS, nparts, parts)
    for bins in (0, 33, True, 2.5):
        with pytest.raises(ValueError, match="bins"):
            slots.voxel(table, pred, 255, bins, nparts, parts)
    for mc in (0, 256, True):
        with pytest.raises(ValueError, match="max_count"):
            slots.voxel(table, pred, mc, BINS, nparts, parts)
    for bad in (0, slots.MAX_EMIT_PARTS + 1, True):
        with pytest.raises(ValueError, match="nparts"):
            slots.voxel(table, pred, 255, BINS, bad, parts)
    with pytest.raises(ValueError, match="parts"):
        slots.voxel(table, pred, 255, BINS, nparts, parts[:2 * S * nparts - 1])
    with pytest.raises(ValueError, match="pred"):
        slots.voxel(table, pred[:S - 1], 255, BINS, nparts, parts)
    torch.cuda.synchronize()
    assert torch.equal(first, buf)


# ------------------------------------------------------------------ (c) sessions
H_, W_ = 12, 20
WINDOWS = (4, 6, 3, 5)
SEED = 31


@functools.lru_cache(maxsize=None)
def _case(H, W, gh, gw, seed):
    return _recordings(WINDOWS, H, W, gh, gw, seed)


@functools.lru_cache(maxsize=None)
def _session(graph, S=3, only=None, gt=True, extra=()):
    """The session with voxel grids on the four recordings (or on recording `only` alone) -> the results per recording."""
    dev = _gpu()
    from infer import MultiStreamSR
    m = _model(False, N_C, seed=307).to(dev)
    recs = [(f.to(dev), g.to(dev)) for f, g in _case(H_, W_, SCALE * H_, SCALE * W_, SEED)]
    if only is not None:
        recs = [recs[only]]
    ms = MultiStreamSR(m, S, n_c=N_C, scale=SCALE, graph=graph, keep_predictions=True, voxel_bins=BINS, **dict(extra))
    room = {}
    if dict(extra).get("emit_events"):                     # room for 16 events per element of every window
        per_window = 16 * 2 * SCALE * H_ * SCALE * W_
        room = dict(event_capacity=max(WINDOWS) * per_window, window_event_capacity=per_window)
    hs = [ms.open(f, g if gt else None, **room) for f, g in recs]
    empty = False
    while ms.step():
        empty |= any(s is None for s in ms.sched.slots)                        # (the slots as the window just run had them)
    if graph:
        assert ms._graph is not None and ms.replays > 0
    if only is None:
        assert empty and len(recs) > S                                         # a slot was reused, and one stood empty
    torch.cuda.synchronize()
    return [ms.results(h) for h in hs]


def _check_voxels(res, nwin, what):
    """A recording's grids against the restatement of its kept predictions; -> (windows with N > 3, any q >= 2, any non-zero)."""
    vox, pred = res["voxels"], _np(res["predictions"])
    assert vox.dtype == torch.float32 and vox.is_cuda and tuple(vox.shape) == (nwin, BINS) + pred.shape[2:] and len(pred) == nwin
    live = big = nonzero = 0
    for i in range(nwin):
        want = V.voxel_np(pred[i], BINS)
        assert _np(vox[i]).tobytes() == want.tobytes(), (what, i)
        q = quantise_np(pred[i])
        live, big, nonzero = live + (q.sum() > 3), big + (q.max() >= 2), nonzero + bool(want.any())
    return live, big, nonzero


@pytest.mark.parametrize("graph", [False, True])
def test_session_voxels_equal_the_restatement(graph):
    res = _session(graph)
    stats = [_check_voxels(r, n, (graph, k)) for k, (r, n) in enumerate(zip(res, WINDOWS))]
    assert all(s[0] > 0 for s in stats)                    # every recording has a window with more than 3 events,
    assert sum(s[1] for s in stats) > 0                    # some window has an element with 2 events or more,
    assert sum(s[2] for s in stats) > 0                    # and some grid is not blank


def test_eager_and_graph_sessions_are_byte_identical():
    for a, b in zip(_session(False), _session(True)):
        assert torch.equal(a["predictions"], b["predictions"]) and torch.equal(a["voxels"], b["voxels"])


def test_a_recording_alone_gives_the_same_grids():
    beside = _session(False)[1]
    alone = _session(False, S=1, only=1)[0]
    assert torch.equal(alone["predictions"], beside["predictions"]) and torch.equal(alone["voxels"], beside["voxels"])


@pytest.mark.parametrize("graph", [False, True])
def test_recordings_without_ground_truth(graph):
    res = _session(graph, gt=False)
    for k, (r, n, with_gt) in enumerate(zip(res, WINDOWS, _session(graph))):
        assert "esr_mse" not in r and _check_voxels(r, n, (graph, k))[0] > 0
        assert torch.equal(r["voxels"], with_gt["voxels"])


@pytest.mark.parametrize("graph", [False, True])
def test_event_backed_filtered_session(graph):
    dev = _gpu()
    from infer import MultiStreamSR
    from test_gpu_hot_filter import GH, GW, HF, _dev, _session_recordings
    from test_gpu_hot_filter import H_ as EH, W_ as EW
    m = _model(False, N_C, seed=313).to(dev)
    recs = _session_recordings()[:3]
    ms = MultiStreamSR(m, 2, n_c=N_C, scale=SCALE, graph=graph, keep_predictions=True, hot_filter=HF, voxel_bins=BINS)
    hs = [ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (EH, EW), (GH, GW)) for lr, li, gt, gi, _ in recs]
    ms.run()
    if graph:
        assert ms.replays > 0
    stats = [_check_voxels(ms.results(h), len(li) - SEQN + 1, (graph, k)) for k, (h, (_, li, _, _, _)) in enumerate(zip(hs, recs))]
    assert all(s[0] > 0 for s in stats) and sum(s[2] for s in stats) > 0


@pytest.mark.parametrize("graph", [False, True])
def test_voxels_beside_the_event_stream(graph):
    """voxel_bins with emit_events and event_times: the same grids, and the grids are those of the stream the session emits."""
    from bmc_hip import encodings
    plain = _session(graph)
    both = _session(graph, extra=(("emit_events", True), ("event_times", "linear")))
    for a, b in zip(plain, both):
        assert torch.equal(a["predictions"], b["predictions"]) and torch.equal(a["voxels"], b["voxels"])
    r = both[1]
    xs, ys, ps = r["sr_events"]
    index = r["sr_index"]
    sH, sW = SCALE * H_, SCALE * W_
    for i in range(WINDOWS[1]):
        lo, hi = int(index[i]), int(index[i + 1])
        want = encodings.events_to_voxel_torch(xs[lo:hi].float(), ys[lo:hi].float(), r["sr_ts"][lo:hi].clone(), ps[lo:hi].float(),
                                               BINS, sensor_size=(sH, sW))
        assert torch.equal(r["voxels"][i], want), i


# ------------------------------------------------------------------ (d) the default, and the bytes
def test_without_voxel_bins_nothing_changes():
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR, evaluate_recordings
    m = _model(False, N_C, seed=317).to(dev)
    recs = [(f.to(dev), g.to(dev)) for f, g in _case(H_, W_, SCALE * H_, SCALE * W_, SEED)][:2]
    sH, sW = SCALE * H_, SCALE * W_

    def session(**kw):
        ms = MultiStreamSR(m, 2, n_c=N_C, scale=SCALE, keep_predictions=True, **kw)
        hs = [ms.open(f, g) for f, g in recs]
        per = []
        while True:
            before = (dict(slots.LAUNCHES), slots.EMIT_LAUNCHES, slots.RENDER_LAUNCHES, slots.VOXEL_LAUNCHES)
            if not ms.step():
                break
            per.append(({k: slots.LAUNCHES[k] - before[0][k] for k in before[0]}, slots.EMIT_LAUNCHES - before[1],
                        slots.RENDER_LAUNCHES - before[2], slots.VOXEL_LAUNCHES - before[3]))
        return ms, hs, per

    one = {"stage": 1, "commit": 1, "metrics": 1}
    without, h0, per0 = session()
    off, h1, per1 = session(voxel_bins=None)
    on, h2, per2 = session(voxel_bins=BINS)
    assert per0 == per1 and all(p == (one, 0, 0, 0) for p in per0)             # VOXEL_LAUNCHES did not move
    assert all(p == (one, 0, 0, 1) for p in per2) and slots.VOXEL_KERNELS == 2  # on: one call (two launches) per window
    for ms in (without, off):
        t = ms._bufs["table"]
        assert not t.voxel and t.dev.numel() == slots.table_layout(2)[1] and "voxel_parts" not in ms._bufs
        assert ms.scratch_bytes() == 0
    assert on._bufs["table"].voxel and on._bufs["table"].dev.numel() == slots.table_layout(2)[1] + 2 * 8
    assert on.scratch_bytes() == 4 * 2 * 2 * slots.voxel_parts(sH, sW)
    for a, b, c, (f, _) in zip(h0, h1, h2, recs):
        ra, rb, rc = without.results(a), off.results(b), on.results(c)
        for r in (ra, rb, rc):
            r.pop("time")
        assert set(ra) == set(rb) == {"esr_mse", "bicubic_mse", "predictions"} and set(rc) == set(ra) | {"voxels"}
        assert ra["esr_mse"] == rb["esr_mse"] == rc["esr_mse"] and ra["bicubic_mse"] == rb["bicubic_mse"] == rc["bicubic_mse"]
        assert torch.equal(ra["predictions"], rb["predictions"]) and torch.equal(ra["predictions"], rc["predictions"])
        assert without.resident_bytes(a) == off.resident_bytes(b)
        nwin = len(f) - SEQN + 1
        assert on.resident_bytes(c) == off.resident_bytes(b) + 4 * BINS * sH * sW * nwin
    out = evaluate_recordings(m, recs, 2, n_c=N_C, scale=SCALE, keep_predictions=True)
    assert "voxels" not in out
    out = evaluate_recordings(m, recs, 2, n_c=N_C, scale=SCALE, voxel_bins=BINS)
    assert set(out["voxels"]) == {"0", "1"} and torch.equal(out["voxels"]["1"], on.results(h2[1])["voxels"])
    with pytest.raises(ValueError, match="voxel_bins"):
        evaluate_recordings(m, recs, 2, n_c=N_C, scale=SCALE, voxel_bins=33)
