"""Hot-pixel filter on the GPU (include/bmc_hip.h, "hot-pixel filter"): the drop-in against the reference's outputs, the update
and the filtered encode launch against the numpy restatement (tests/hot_filter_ref.py), and filtered event-backed sessions
against open() on the restatement's filtered frames -- all byte for byte."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hot_filter_ref as R
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_multistream import SCALE, SEQN, _model
from test_hot_filter_cpu import golden_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


# ------------------------------------------------------------------ (a) the drop-in
def test_get_hot_event_mask_equals_the_reference():
    dev = _gpu()
    from bmc_hip.encodings import get_hot_event_mask
    n = 0
    for k, rate, idx, max_px, min_obvs, max_rate, mask, after in golden_cases():
        t = torch.tensor(rate).to(dev)
        m = get_hot_event_mask(t, idx, max_px=max_px, min_obvs=min_obvs, max_rate=max_rate)
        assert m.dtype == torch.float32 and m.shape == t.shape
        assert m.cpu().numpy().tobytes() == mask.tobytes(), (k, idx, max_px, min_obvs, max_rate)
        assert t.cpu().numpy().tobytes() == after.tobytes(), (k, idx, max_px, min_obvs, max_rate)
        n += 1
    assert n >= 36
    t = torch.tensor([[0.9, 0.1], [0.95, 0.85]], device=dev)                  # the defaults are the reference's
    assert get_hot_event_mask(t, 6).cpu().tolist() == [[0.0, 1.0], [0.0, 0.0]]
    assert torch.equal(t.cpu(), torch.tensor([[0.0, 0.1], [0.0, 0.0]]))       # (float32 0.1 on both sides)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        get_hot_event_mask(torch.zeros(2, 2), 9)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        get_hot_event_mask(torch.zeros(2, 2, device=dev, dtype=torch.float64), 9)


def _bits(words):
    return np.asarray(words, np.uint32).view(np.float32)


def _tie_cases():
    """(name, rate [37, 53], max_px): more candidates than max_px on a frame of 1 961 pixels (two per lane of the select's
    workgroup), so the radix select runs and keys equal to the threshold T must be cut in flat order."""
    H, W = 37, 53
    n = H * W
    yield "uniform", np.full((H, W), 0.9, np.float32), 5                      # every key == T; the cut falls inside a lane's chunk
    flat = np.full(n, 0.1, np.float32)                                        # T's keys over the waves, at both places of a chunk
    ties = np.arange(3, n, 97)
    flat[ties] = 0.9
    flat[[130, 777, 1500]] = 0.95
    assert len(ties) == 21 and len(set(ties // 128)) >= 10 and len(set(ties % 2)) == 2
    yield "spread", flat.reshape(H, W), 3 + 11
    # T = 0x3F6600FF: the select's third pass picks digit 0 (digit 1 above it), its fourth digit 255 (smaller digits below it)
    rng = np.random.default_rng(5)
    flat = np.full(n, 0.1, np.float32)
    pos = rng.permutation(n)
    flat[pos[:40]] = _bits(0x3F660100 + rng.integers(0, 256, 40))
    flat[pos[40:70]] = _bits([0x3F6600FF] * 30)
    flat[pos[70:270]] = _bits(0x3F660000 + rng.integers(0, 255, 200))
    assert flat[pos[:270]].min() > np.float32(0.8)
    yield "digit_ends", flat.reshape(H, W), 40 + 13


def test_get_hot_event_mask_cuts_ties_in_flat_order():
    """Ties at the threshold of the radix select, against the restatement of the reference's loop, byte for byte."""
    dev = _gpu()
    from bmc_hip.encodings import get_hot_event_mask
    for name, rate, max_px in _tie_cases():
        want_mask, want_after = R.get_hot_event_mask_np(rate, 9, max_px, 5, 0.8)
        assert (want_mask == 0).sum() == max_px < (rate > np.float32(0.8)).sum(), name
        t = torch.tensor(rate).to(dev)
        m = get_hot_event_mask(t, 9, max_px=max_px, min_obvs=5, max_rate=0.8)
        assert m.cpu().numpy().tobytes() == want_mask.tobytes(), name
        assert t.cpu().numpy().tobytes() == want_after.tobytes(), name


# ------------------------------------------------------------------ (b) bmc_slot_hot_update
PARAMS = {"ties": (3, 2, 0.6), "max_px_0": (0, 2, 0.6), "negative_rate": (1 << 20, 1, -0.5), "rate_1": (7, 1, 1.0),
          "all_active": (100, 1, 0.5)}


@functools.lru_cache(maxsize=None)
def _update_case(H, W, kind):
    """Three planted recordings A, B (slot 0: A, then B after a reset) and C (slot 1) and their restatements."""
    rng = np.random.default_rng(H * 1000 + W)
    hot = [(0, 0), (H // 2, W // 3), (H - 1, W - 1), (1, 1 % W), (H // 3, W // 2)]
    recs = []
    for L, kw in ((6, dict(empty_item=2)), (5, dict(zero_last=(3, 1))), (9, dict(empty_item=7, zero_last=(5, 2)))):
        if kind == "all_active":                                              # every pixel fires in every item
            n = H * W
            index = np.array([(j * n, (j + 1) * n) for j in range(L)], np.int64)
            lr = (np.tile(np.arange(n) % W, L).astype(np.int16), np.tile(np.arange(n) // W, L).astype(np.int16), np.ones(L * n))
        else:
            lr, index = R.planted_recording(rng, (H, W), L, max(H * W // 40, 5), hot, **kw)
        recs.append((lr, index, R.filter_recording_np(lr, index, (H, W), *PARAMS[kind])))
    return recs


def _guarded(n, dtype, fill, dev):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


@pytest.mark.parametrize("kind", list(PARAMS))
@pytest.mark.parametrize("H,W,S", [(5, 7, 1), (37, 53, 3), (180, 240, 2)])
def test_hot_update_window_by_window(H, W, S, kind):
    dev = _gpu()
    from bmc_hip import slots
    max_px, min_obvs, max_rate = PARAMS[kind]
    A, B, C = _update_case(H, W, kind)
    if kind == "ties":             # the inputs fire the filter: ties above max_px, windows on both sides of min_obvs, masks
        for _, _, f in (A, B, C):
            assert (f["hot"][:min_obvs] == 0).all() and f["hot"][min_obvs:].max() == max_px
        cmin = R.cmin_np(9, max_rate)
        assert (C[2]["counts"][8] >= cmin).sum() > max_px and (C[2]["masks"] == 0).any()
        assert C[2]["counts"][1][0, 0] < 2                                    # an out-of-range event cleared pixel (0, 0)
    if kind == "negative_rate":
        assert (A[2]["masks"][2] == 0).sum() == (A[2]["counts"][2] > 0).sum() + (A[2]["counts"][2][0, 0] == 0)
    if kind == "rate_1":
        assert all((f["masks"] == 1).all() for _, _, f in (A, B, C))
    if kind == "all_active":
        assert (C[2]["masks"][4].reshape(-1) == 0).nonzero()[0].tolist() == list(range(min(100, H * W)))
    n = H * W
    table = slots.SlotTable(S, dev, events=True, hot=True)
    cbuf, counts = _guarded(S * n, torch.int32, 12345, dev)
    rbuf, ring = _guarded(S * SEQN * n, torch.uint8, 7, dev)
    wbuf, ws = _guarded(S * n, torch.int32, 999, dev)
    counts, ring, ws = counts.view(S, H, W), ring.view(S, SEQN, H, W), ws.view(S, H, W)
    plan0 = [(A, i) for i in range(4)] + [(B, i) for i in range(3)]           # slot 0: A's windows, then B from a reset
    plan1 = [(C, i) for i in range(7)]
    outs = {}
    for k, (lr, index, f) in enumerate((A, B, C)):
        outs[k] = dict(cols=tuple(torch.tensor(c).to(dev) for c in lr), px=_guarded(len(index) - SEQN + 1, torch.int32, -5, dev),
                       mask=_guarded(n, torch.uint8, 9, dev))
    ids = {id(A): 0, id(B): 1, id(C): 2}
    for step in range(7):
        table.host()
        ev, ht = table.events_host(), table.hot_host()
        active = [(0, plan0[step])] + ([(1, plan1[step])] if S > 1 else [])  # with S = 3 the last slot is never active
        for s, (rec, i) in active:
            o = outs[ids[id(rec)]]
            for key, t in zip(("lr_xs", "lr_ys", "lr_ps"), o["cols"]):
                ev[key][s] = t.data_ptr()
            ev["lr_range"][s, :SEQN] = rec[1][i:i + SEQN]
            ht[s]["active"], ht[s]["first_item"], ht[s]["new_from"] = 1, i, 0 if i == 0 else SEQN - 1
            ht[s]["cmin"][:SEQN] = [slots.hot_cmin(j + 1, min_obvs, max_rate) for j in range(i, i + SEQN)]
            ht[s]["hot_pixels"], ht[s]["hot_mask"] = o["px"][1].data_ptr() + 4 * i, o["mask"][1].data_ptr()
        table.upload()
        before = slots.HOT_LAUNCHES
        slots.hot_update(table, counts, ring, ws, max_px, max_rate)
        assert slots.HOT_LAUNCHES == before + 1
        torch.cuda.synchronize()
        for s, (rec, i) in active:
            f, o = rec[2], outs[ids[id(rec)]]
            last = i + SEQN - 1
            assert counts[s].cpu().numpy().tobytes() == f["counts"][last].tobytes(), (step, s)
            want = np.empty((SEQN, H, W), np.uint8)
            for j in range(i, i + SEQN):
                want[j % SEQN] = f["masks"][j]
            assert ring[s].cpu().numpy().tobytes() == want.tobytes(), (step, s)
            assert o["px"][1][:i + 1].cpu().tolist() == f["hot"][SEQN - 1:last + 1].tolist(), (step, s)
            assert o["mask"][1].cpu().numpy().tobytes() == f["masks"][last].tobytes(), (step, s)
        for s in range(len(active), S):                                       # an inactive slot stays untouched
            assert (counts[s] == 12345).all() and (ring[s] == 7).all() and (ws[s] == 999).all()
    if S == 1:                                                                # ... and so does a slot whose entry went inactive
        snap = [t.clone() for t in (cbuf, rbuf, wbuf)]
        table.host()
        table.upload()
        slots.hot_update(table, counts, ring, ws, max_px, max_rate)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(snap, (cbuf, rbuf, wbuf)))
    for buf, fill in ((cbuf, 12345), (rbuf, 7), (wbuf, 999)) + tuple((o["px"][0], -5) for o in outs.values()) + \
            tuple((o["mask"][0], 9) for o in outs.values()):
        assert (buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all()


# ------------------------------------------------------------------ (c) bmc_slot_encode_filtered
@pytest.mark.parametrize("H,W", [(10, 16), (37, 53)])
def test_encode_filtered_bit_exact(H, W):
    """Slot 0 filtered, slot 1 event-backed but not filtered (== bmc_slot_encode), slot 2 without an event entry (untouched)."""
    dev = _gpu()
    from bmc_hip import slots
    from test_gpu_event_slots import _columns
    rng = np.random.default_rng(H)
    S, gh, gw = 3, SCALE * H, SCALE * W - 2
    lr, index = R.planted_recording(rng, (H, W), 6, 3 * H * W, [(0, 0), (H - 1, 2)], oob=12)
    gt = _columns(rng, 500, gh, gw)
    cols = tuple(torch.tensor(c).to(dev) for c in lr + gt)
    first = 2                                                                 # the window of items 2, 3, 4
    masks = (rng.random((SEQN, H, W)) < 0.7).astype(np.uint8)                 # ring position p holds the mask of item p mod SEQN
    masks[:, 0, 0] = 0                                                        # the out-of-range negatives on [H-1][0] go
    rbuf, ring = _guarded(S * SEQN * H * W, torch.uint8, 1, dev)
    ring = ring.view(S, SEQN, H, W)
    ring[0] = torch.tensor(masks).to(dev)
    ring[1] = 0                                                               # (not read: slot 1 is not filtered)
    table = slots.SlotTable(S, dev, events=True, hot=True)
    table.host()
    ev, ht = table.events_host(), table.hot_host()
    for s in (0, 1):
        for key, t in zip(("lr_xs", "lr_ys", "lr_ps", "gt_xs", "gt_ys", "gt_ps"), cols):
            ev[key][s] = t.data_ptr()
        ev["lr_range"][s, :SEQN] = index[first:first + SEQN]
        ev["gt_range"][s] = (17, 480)
    ht[0]["active"], ht[0]["first_item"], ht[0]["new_from"] = 1, first, SEQN - 1
    table.upload()
    lbuf, lr_s = _guarded(S * SEQN * 2 * H * W, torch.float32, -3.0, dev)
    gbuf, gt_s = _guarded(S * 2 * gh * gw, torch.float32, -3.0, dev)
    lr_s, gt_s = lr_s.view(S, SEQN, 2, H, W), gt_s.view(S, 2, gh, gw)
    plain_l, plain_g = torch.full_like(lr_s, -3.0), torch.full_like(gt_s, -3.0)
    before = slots.ENCODE_LAUNCHES
    slots.encode_filtered(table, lr_s, gt_s, ring)
    assert slots.ENCODE_LAUNCHES == before + 1
    slots.encode(table, plain_l, plain_g)
    torch.cuda.synchronize()
    raw = np.stack([R.O.encode_raw_frame_np(*(c[a:b] for c in lr), 0, (H, W)) for a, b in index[first:first + SEQN]])
    assert raw[:, 1, H - 1, 0].min() > 0                                      # out-of-range negatives did land there
    want = np.stack([raw[t] * masks[(first + t) % SEQN][::-1][None].astype(np.float32) for t in range(SEQN)])
    assert plain_l[0].cpu().numpy().tobytes() == raw.tobytes()
    assert lr_s[0].cpu().numpy().tobytes() == want.tobytes() and not np.array_equal(want, raw)
    assert torch.equal(lr_s[1], plain_l[1]) and torch.equal(gt_s[:2], plain_g[:2])
    assert (lr_s[2] == -3.0).all() and (gt_s[2] == -3.0).all()
    for buf, fill in ((lbuf, -3.0), (gbuf, -3.0), (rbuf, 1)):
        assert (buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all()
    with pytest.raises(ValueError, match="no hot entries"):
        slots.encode_filtered(slots.SlotTable(S, dev, events=True), lr_s, gt_s, ring)


# ------------------------------------------------------------------ (d) sessions
HF = dict(max_px=3, min_obvs=1, max_rate=0.6)
H_, W_ = 10, 16
GH, GW = SCALE * H_, SCALE * W_ - 2


@functools.lru_cache(maxsize=None)
def _session_recordings():
    """Six event recordings of 6-8 windows with five planted hot pixels -> (lr, index, gt, gt_index, restatement) each."""
    from test_gpu_event_slots import _columns
    out = []
    for k, nwin in enumerate([6, 8, 7, 6, 8, 7]):
        rng = np.random.default_rng(900 + k)
        L = nwin + SEQN - 1
        hot = [(0, 0), (3, 5), (9, 15), (4, 4), (7, 1)]
        lr, index = R.planted_recording(rng, (H_, W_), L, 40, hot, empty_item=3 if k == 1 else None)
        gt = _columns(rng, 300 * L, GH, GW)
        gt_index = np.array([(300 * j, 300 * (j + 1)) for j in range(L)], np.int64)
        f = R.filter_recording_np(lr, index, (H_, W_), HF["max_px"], HF["min_obvs"], HF["max_rate"])
        assert f["hot"].max() == 3 and not np.array_equal(f["frames"], f["raw"])
        out.append((lr, index, gt, gt_index, f))
    return out


def _dev(cols, dev):
    return tuple(torch.tensor(c).to(dev) for c in cols)


def _gt_frames(gt, gt_index, dev):
    from test_gpu_event_slots import _encode_frames
    return _encode_frames(gt, gt_index, GH, GW, dev)


def _equal_results(a, b, emit):
    assert a["esr_mse"] == b["esr_mse"] and a["bicubic_mse"] == b["bicubic_mse"] and len(a["esr_mse"]) > 0
    assert torch.equal(a["predictions"], b["predictions"])
    if emit:
        assert torch.equal(a["sr_index"], b["sr_index"]) and all(torch.equal(x, y) for x, y in zip(a["sr_events"], b["sr_events"]))


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("plain", [False, True])
def test_filtered_session_equals_frames_filtered_on_the_cpu(plain, graph, S):
    dev = _gpu()
    from infer import MultiStreamSR
    n_c = 16
    m = _model(plain, n_c, seed=211).to(dev)
    recs = _session_recordings()[:3 if S == 1 else 6]
    emit = not plain
    kw = dict(n_c=n_c, scale=SCALE, plain=plain, graph=graph, keep_predictions=True, emit_events=emit)
    cap = dict(event_capacity=300000) if emit else {}
    gts = [_gt_frames(gt, gi, dev) for _, _, gt, gi, _ in recs]

    def run_events(hot_filter):
        ms = MultiStreamSR(m, S, hot_filter=hot_filter, **kw)
        hs = [ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H_, W_), (GH, GW), **cap) for lr, li, gt, gi, _ in recs]
        ms.run()
        if graph:
            assert ms._graph is not None and ms.replays > 0
        return [ms.results(h) for h in hs]

    ref = MultiStreamSR(m, S, **kw)
    hr = [ref.open(torch.tensor(f["frames"]).to(dev), g, **cap) for (_, _, _, _, f), g in zip(recs, gts)]
    ref.run()
    first, second, off = run_events(HF), run_events(HF), run_events(None)
    differs = False
    for a, a2, u, h, (_, li, _, _, f) in zip(first, second, off, hr, recs):
        _equal_results(a, ref.results(h), emit)
        _equal_results(a, a2, emit)                                           # the same bytes run after run
        assert a["hot_pixels"] == a2["hot_pixels"] == f["hot"][SEQN - 1:].tolist()
        assert a["hot_mask"].cpu().numpy().tobytes() == f["masks"][-1].tobytes()
        assert "hot_pixels" not in u and "hot_mask" not in u
        differs |= not torch.equal(a["predictions"], u["predictions"])
    assert differs                                                            # the filter acted


@pytest.mark.parametrize("graph", [False, True])
def test_mixed_filtered_session(graph):
    """A frame-backed recording (unfiltered), a filtered event recording and one without ground truth share 2 slots."""
    dev = _gpu()
    from infer import EventRecording, MultiStreamSR, evaluate_recordings
    n_c = 16
    m = _model(False, n_c, seed=223).to(dev)
    (lr0, li0, gt0, gi0, f0), (lr1, li1, gt1, gi1, f1), (lr2, li2, gt2, gi2, f2) = _session_recordings()[:3]
    kw = dict(n_c=n_c, scale=SCALE, graph=graph, keep_predictions=True)
    g0, g1 = _gt_frames(gt0, gi0, dev), _gt_frames(gt1, gi1, dev)
    raw0 = torch.tensor(f0["raw"]).to(dev)
    ms = MultiStreamSR(m, 2, hot_filter=HF, **kw)
    hs = [ms.open(raw0, g0), ms.open_events(_dev(lr1, dev), _dev(gt1, dev), li1, gi1, (H_, W_), (GH, GW)),
          ms.open_events(_dev(lr2, dev), None, li2, None, (H_, W_))]
    ms.run()
    ref = MultiStreamSR(m, 2, **kw)
    hr = [ref.open(raw0, g0), ref.open(torch.tensor(f1["frames"]).to(dev), g1), ref.open(torch.tensor(f2["frames"]).to(dev))]
    ref.run()
    for k, (a, b) in enumerate(zip(hs, hr)):
        ra, rb = ms.results(a), ref.results(b)
        assert torch.equal(ra["predictions"], rb["predictions"]) and ra.get("esr_mse") == rb.get("esr_mse")
        assert ra.get("bicubic_mse") == rb.get("bicubic_mse") and ("hot_pixels" in ra) == (k > 0)
    assert "esr_mse" not in ms.results(hs[2]) and ms.results(hs[2])["hot_pixels"] == f2["hot"][SEQN - 1:].tolist()
    out = evaluate_recordings(m, [EventRecording(_dev(lr1, dev), _dev(gt1, dev), li1, gi1, (H_, W_), (GH, GW))], 1,
                              hot_filter=HF, **kw)
    assert torch.equal(out["predictions"]["0"], ref.results(hr[1])["predictions"])
    with pytest.raises(ValueError, match="max_rate"):
        evaluate_recordings(m, [(raw0, g0)], 1, hot_filter=dict(HF, max_rate=float("nan")), **kw)


# ------------------------------------------------------------------ (e) launch accounting, (f) bytes
def test_launches_and_bytes():
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    n_c, S = 16, 2
    m = _model(False, n_c, seed=227).to(dev)
    recs = _session_recordings()[:2]

    def session(**kw):
        ms = MultiStreamSR(m, S, n_c=n_c, scale=SCALE, keep_predictions=True, **kw)
        hs = [ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H_, W_), (GH, GW)) for lr, li, gt, gi, _ in recs]
        per = []
        while True:
            before = (dict(slots.LAUNCHES), slots.ENCODE_LAUNCHES, slots.HOT_LAUNCHES)
            if not ms.step():
                break
            per.append(({k: slots.LAUNCHES[k] - before[0][k] for k in before[0]}, slots.ENCODE_LAUNCHES - before[1],
                        slots.HOT_LAUNCHES - before[2]))
        return ms, hs, per

    one = {"stage": 1, "commit": 1, "metrics": 1}
    without, h0, per0 = session()
    off, h1, per1 = session(hot_filter=None)
    on, h2, per2 = session(hot_filter=HF)
    assert per0 == per1 and all(p == (one, 1, 0) for p in per0)               # off: the launches of a session without the argument
    assert all(p == (one, 1, slots.HOT_KERNELS) for p in per2) and slots.HOT_KERNELS == 1     # on: ONE more launch per window
    for a, b in zip(h0, h1):
        ra, rb = without.results(a), off.results(b)
        ra.pop("time"), rb.pop("time")
        assert set(ra) == set(rb) == {"esr_mse", "bicubic_mse", "predictions"}
        assert ra["esr_mse"] == rb["esr_mse"] and ra["bicubic_mse"] == rb["bicubic_mse"] and torch.equal(ra["predictions"], rb["predictions"])
    assert "hot_ring" not in off._bufs and not off._bufs["table"].hot and off._bufs["table"].dev.numel() == without._bufs["table"].dev.numel()
    scratch = 4 * S * (SEQN * 2 * H_ * W_ + 2 * GH * GW)
    assert off.scratch_bytes() == without.scratch_bytes() == scratch
    assert on.scratch_bytes() == scratch + S * H_ * W_ * (4 + 4 + SEQN)
    b = on._bufs
    assert on.scratch_bytes() == sum(b[k].numel() * b[k].element_size() for k in ("lr_scratch", "gt_scratch", "hot_counts", "hot_ring", "hot_ws"))
    for k, (lr, li, gt, gi, _) in enumerate(recs):
        nwin = len(li) - SEQN + 1
        assert on.resident_bytes(h2[k]) == off.resident_bytes(h1[k]) + 4 * nwin + H_ * W_
    # the buffers first come to exist in a running (captured) frames-only session: the graph is captured again
    ms = MultiStreamSR(m, S, n_c=n_c, scale=SCALE, graph=True, hot_filter=HF)
    f = recs[0][4]
    ms.open(torch.tensor(f["raw"]).to(dev), _gt_frames(recs[0][2], recs[0][3], dev))
    for _ in range(3):
        ms.step()
    assert ms._graph is not None and ms.scratch_bytes() == 0
    lr, li, gt, gi, _ = recs[1]
    ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H_, W_), (GH, GW))
    assert ms._graph is None and "hot_ring" in ms._bufs
    ms.run()
    assert ms._graph is not None
    with pytest.raises(ValueError, match="2\\^23"):
        big = np.zeros((1 << 23, 2), np.int64)
        MultiStreamSR(m, S, n_c=n_c, scale=SCALE, hot_filter=HF).open_events(_dev(lr, dev), None, big, None, (H_, W_))


# ------------------------------------------------------------------ (g) the tool
def test_tool_hot_filter_row_parses():
    _gpu()
    import json
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "multistream_infer.py"), "--hot-filter", "--sizes", "31x56",
                        "--slots", "2", "--windows", "2", "--warmup", "3", "--modes", "graph", "--runs", "1"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    rows = [json.loads(ln) for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    row = next(r for r in rows if r.get("hot_filter"))
    assert row["events"] and row["windows_per_s"] > 0 and row["windows_per_s_filter_off"] > 0 and row["hot_update_alone_ms"] > 0
    assert row["hot_filter"] == {"max_px": 100, "min_obvs": 5, "max_rate": 0.8}
