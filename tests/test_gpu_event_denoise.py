"""The background-activity noise filter on the GPU (include/bmc_hip_denoise.h): the entry point, the order inside a step and the
contract's corners byte for byte against the sequential restatement (tests/event_denoise_ref.py); filtered sessions and training
sets against the same recordings filtered by the restatement before they are handed over."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import event_denoise_ref as R
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def _guarded(n, dtype, fill, dev):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, fill):
    edge = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool(torch.isnan(edge).all()) if isinstance(fill, float) and math.isnan(fill) else bool((edge == fill).all())


def _call(dev, cols, H, W, dt, k, keep=True, ps_out=True, kept=True):
    """bmc_event_denoise on numpy columns with every output pre-filled (0xFF / NaN / -1) inside guard regions -> (keep, ps_out,
    kept) as numpy / int, None for an output passed as NULL; the guards and the input columns are checked untouched."""
    from bmc_hip import denoise_lib, lib, ops
    xs, ys, ts, ps = (torch.tensor(c).to(dev) for c in cols)
    before = [t.clone() for t in (xs, ys, ts, ps)]
    n = xs.numel()
    nb = denoise_lib.scratch_bytes(H, W) // 8
    assert nb == -(-H // denoise_lib.band_rows(H, W)) >= 1
    kb, kv = _guarded(n, torch.uint8, 0xFF, dev)
    pb, pv = _guarded(n, torch.float64, float("nan"), dev)
    cb, cv = _guarded(1, torch.int64, -1, dev)
    sb, sv = _guarded(nb, torch.int64, -1, dev)
    lib.call(denoise_lib._event_denoise, "bmc_event_denoise", xs.data_ptr(), ys.data_ptr(), ts.data_ptr(), ps.data_ptr(), n, H, W,
             float(dt), int(k), kv.data_ptr() if keep else None, pv.data_ptr() if ps_out else None, cv.data_ptr() if kept else None,
             sv.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert _intact(kb, 0xFF) and _intact(pb, float("nan")) and _intact(cb, -1) and _intact(sb, -1)
    assert all(torch.equal(a, b) for a, b in zip(before, (xs, ys, ts, ps)))
    if not keep:
        assert bool((kv == 0xFF).all())
    if not ps_out:
        assert bool(torch.isnan(pv).all())
    if not kept:
        assert int(cv[0]) == -1 and bool((sv == -1).all())
    return (kv.cpu().numpy() if keep else None, pv.cpu().numpy() if ps_out else None, int(cv[0]) if kept else None)


def _agrees(dev, cols, H, W, dt, k, want=None, **outputs):
    xs, ys, ts, ps = cols
    if want is None:
        want = R.mask_seq(xs, ys, ts, H, W, dt, k)
    keep, ps_out, kept = _call(dev, cols, H, W, dt, k, **outputs)
    if keep is not None:
        assert keep.tobytes() == want.tobytes(), (H, W, len(xs), dt, k, np.flatnonzero(keep != want)[:8])
    if ps_out is not None:                                   # +0.0 where dropped: the bytes, not the values
        assert ps_out.tobytes() == np.where(want == 1, ps, 0.0).tobytes()
    if kept is not None:
        assert kept == int(want.sum())
    return want


# ------------------------------------------------------------------ 1. the entry point, byte for byte
def _max_w():
    from bmc_hip import denoise_lib
    return denoise_lib.MAX_W


SHAPES = [(1, 1, 50, 0.2), (1, 9, 200, 2e-2), (5, 7, 0, 2e-2), (5, 7, 1, 2e-2), (5, 7, 255, 2e-2), (5, 7, 256, 2e-2), (5, 7, 257, 2e-2),
          (5, 7, 600, 2e-2), (37, 53, 6000, 1e-2), (180, 240, 100000, 2e-3), (7, "max", 20000, 5e-3)]


@functools.lru_cache(maxsize=None)
def _case(H, W, n, dt, k):
    """The stream of a generated case and the restatement's mask, computed once; support 8 runs on a dense stream (all noise,
    a dt longer than the stream: the full ring fills up as the surface does) and asserts only that both outcomes occur."""
    dense = k == 8
    cols = R.stream(H, W, n, 1.0 if dense else 0.3, seed=H * W + n + 1)
    dt = 10.0 if dense else dt
    want = R.mask_seq(*cols[:3], H, W, dt, k)
    return cols, dt, want


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("H,W,n,dt", SHAPES, ids=lambda v: str(v))
def test_entry_point_equals_the_restatement(H, W, n, dt, k):
    dev = _gpu()
    from bmc_hip import denoise_lib
    W = denoise_lib.MAX_W if W == "max" else W
    if W == denoise_lib.MAX_W:
        assert denoise_lib.band_rows(H, W) == 3 == denoise_lib.LDS_WORDS // (W + 2) - 2 and H % 3      # the smallest band, ragged
    if (H, W) == (180, 240):
        assert 1 < denoise_lib.band_rows(H, W) < H and H % denoise_lib.band_rows(H, W)                # several bands, ragged
    cols, dt, want = _case(H, W, n, dt, k)
    if k == 8 and H >= 3 and W >= 3 and n >= 600:
        assert 0 < want.sum() < n, (H, W, n, want.mean())
    elif k < 8 and n >= 200:
        assert 0.05 <= want.mean() <= 0.95, (H, W, n, k, want.mean())
    print("kept share %.3f" % (want.mean() if n else 0.0))
    _agrees(dev, cols, H, W, dt, k, want)
    if k == 2:                                               # each output NULL in turn
        for off in ("keep", "ps_out", "kept"):
            _agrees(dev, cols, H, W, dt, k, want, **{off: False})


def test_many_bands_against_the_sorted_form_on_the_gpu():
    """720 x 1280, 200 000 events: 80 bands.  The reference is mask_sorted on the GPU, which the CPU tests tie to mask_seq."""
    dev = _gpu()
    from bmc_hip import denoise_lib
    H, W, n, dt = 720, 1280, 200000, 2e-3
    assert -(-H // denoise_lib.band_rows(H, W)) == 80
    cols = R.stream(H, W, n, 0.3, seed=H * W + n + 1)
    xs, ys, ts = (torch.tensor(c).to(dev) for c in cols[:3])
    for k in (1, 2):
        want = R.mask_sorted(xs, ys, ts, H, W, dt, k).cpu().numpy()
        assert 0.05 <= want.mean() <= 0.95, (k, want.mean())
        _agrees(dev, cols, H, W, dt, k, want)


# ------------------------------------------------------------------ 2. order inside a step
def _planted(n, where):
    """n events 1e-6 apart, all out of range (they touch nothing) but those of `where` = {index: (x, y)}."""
    xs, ys = np.full(n, -1, np.int16), np.full(n, -1, np.int16)
    for i, (x, y) in where.items():
        xs[i], ys[i] = x, y
    return xs, ys, np.arange(n, dtype=np.float64) * 1e-6, np.where(np.arange(n) % 2 == 0, 1.0, -1.0)


def _expect(dev, H, W, where, kept, n=None):
    from bmc_hip import denoise_lib
    n = n or 3 * denoise_lib.STEP + 7
    cols = _planted(n, where)
    want = np.zeros(n, np.uint8)
    want[list(kept)] = 1
    assert np.array_equal(R.mask_seq(*cols[:3], H, W, 1.0, 1), want)      # the hand-written expectation is the contract's
    _agrees(dev, cols, H, W, 1.0, 1, want)


def _pairs(H, W):
    """(p, q) neighbour pixels (x, y): inside one band and, for a sensor of several bands, across the first band boundary in
    both directions (q is then in the halo of p's band only), straight and diagonal."""
    from bmc_hip import denoise_lib
    r = denoise_lib.band_rows(H, W)
    out = [((3, 2), (4, 2)), ((3, 2), (2, 1))]
    if r < H:
        out += [((5, r - 1), (5, r)), ((5, r), (5, r - 1)), ((5, r - 1), (6, r)), ((5, r), (4, r - 1)), ((0, r), (0, r - 1)),
                ((W - 1, r - 1), (W - 1, r))]
    return out


@pytest.mark.parametrize("H,W", [(5, 7), (180, 240), (7, "max")], ids=str)
def test_order_inside_a_step(H, W):
    dev = _gpu()
    from bmc_hip import denoise_lib
    S = denoise_lib.STEP
    W = denoise_lib.MAX_W if W == "max" else W
    for p, q in _pairs(H, W):
        _expect(dev, H, W, {S - 1: q, S: p}, [S])                                    # the previous step's last lane supports
        _expect(dev, H, W, {S + 3: q, S + 100: p}, [S + 100])                        # the same step, an earlier lane
        _expect(dev, H, W, {S + 10: p, S + 200: q}, [S + 200])                       # a later lane must not support p (p does q)
        _expect(dev, H, W, {S + 3: q, S + 100: p, S + 200: q}, [S + 100, S + 200])   # lane 200 hides lane 3 from lane 100
        _expect(dev, H, W, {3: q, S + 100: p, S + 200: q}, [S + 100, S + 200])       # ... hides an earlier STEP's event
        _expect(dev, H, W, {S + 100: p, S + 200: q, S + 201: q}, [S + 200, S + 201]) # hidden, and nothing earlier to find
        _expect(dev, H, W, {**{i: q for i in range(S)}, S: p}, [S])                  # 256 events at one pixel, then its neighbour
        _expect(dev, H, W, {**{5 + i: q for i in range(S)}, S + 5: p}, [S + 5])      # ... astride a step boundary
        _expect(dev, H, W, {**{i: p for i in range(S)}, 7: q}, list(range(7, S)))    # ... the neighbour in their middle
        _expect(dev, H, W, {S + 1: p, S + 2: p, S + 3: p}, [])                       # a pixel never supports itself


# ------------------------------------------------------------------ 3. contract corners
def test_ties_zero_dt_one_ulp_and_epoch_timestamps():
    dev = _gpu()
    H, W, n = 37, 53, 6000
    xs, ys, ts, ps = R.stream(H, W, n, 0.3, seed=5)
    tied = (np.floor(ts * 50) / 50).astype(np.float64)                    # 50 distinct values: long runs of equal timestamps
    for t, dt in ((tied, 0.0), (tied, 0.02), (np.zeros(n), 0.0)):
        want = _agrees(dev, (xs, ys, t, ps), H, W, dt, 1)
        assert 0 < want.sum() < n
    epoch = 1.7e9 + ts                                                    # epoch seconds with microsecond ticks
    assert (np.diff(epoch) >= 0).all() and len(np.unique(epoch)) > n // 2
    want = _agrees(dev, (xs, ys, epoch, ps), H, W, 1e-2, 1)
    assert 0.05 <= want.mean() <= 0.95
    a, b = 1.7e9 + 0.1, 1.7e9 + 0.3
    d = b - a
    two = (np.array([2, 3], np.int16), np.array([2, 2], np.int16), np.array([a, b]), np.array([1.0, -1.0]))
    for dt, kept in ((d, [0, 1]), (np.nextafter(d, 0.0), [0, 0]), (np.nextafter(d, 1.0), [0, 1])):
        want = np.array(kept, np.uint8)
        assert np.array_equal(R.mask_seq(*two[:3], 5, 7, dt, 1), want)
        _agrees(dev, two, 5, 7, dt, 1, want)


def test_refusals():
    dev = _gpu()
    from bmc_hip import denoise_lib, lib
    from bmc_hip.encodings import check_noise_filter, event_noise_mask
    p = torch.zeros(64, dtype=torch.int64, device=dev).data_ptr()         # never read: every call returns at its argument check
    good = dict(xs=p, ys=p, ts=p, ps=p, n=4, H=5, W=7, dt=0.1, k=1, keep=p, ps_out=p, kept=p, scratch=p, s=None)
    for kw in (dict(n=1 << 31), dict(n=-1), dict(W=denoise_lib.MAX_W + 1), dict(W=0), dict(H=0), dict(k=0), dict(k=9), dict(dt=-1e-9),
               dict(dt=math.inf), dict(dt=math.nan), dict(xs=None), dict(ts=None), dict(ps=None), dict(scratch=None)):
        assert denoise_lib._event_denoise(*{**good, **kw}.values()) == -1 and b"bmc_event_denoise" in lib.bmc_last_error(), kw
    assert denoise_lib._event_denoise(*{**good, "W": denoise_lib.MAX_W, "n": 0, "xs": None, "ys": None, "ts": None}.values()) == 0
    assert denoise_lib.band_rows(5, denoise_lib.MAX_W + 1) == -1 == denoise_lib.scratch_bytes(0, 7)
    xs, ys, ts, ps = (torch.tensor(c).to(dev) for c in R.stream(5, 7, 100, 0.3, seed=1))
    bad = ts.clone()
    bad[40] = bad[39] - 1e-6
    nan = ts.clone()
    nan[99] = float("nan")
    for t in (bad, nan, torch.full_like(ts, float("inf"))):
        with pytest.raises(ValueError, match="finite and non-decreasing"):
            check_noise_filter("t: ", dict(ts=t, dt=0.1), (xs, ys, ps), (5, 7))
    assert check_noise_filter("t: ", dict(ts=ts, dt=0.1, support=np.int64(3)), (xs, ys, ps), (5, 7)) == (ts, 0.1, 3)
    with pytest.raises(ValueError, match="one device"):
        check_noise_filter("t: ", dict(ts=ts.cpu(), dt=0.1), (xs, ys, ps), (5, 7))
    with pytest.raises(ValueError, match="at most %d wide" % denoise_lib.MAX_W):
        event_noise_mask(xs, ys, ts, (5, denoise_lib.MAX_W + 1), 0.1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        event_noise_mask(xs.cpu(), ys.cpu(), ts.cpu(), (5, 7), 0.1)


def test_same_bytes_run_after_run_on_any_stream_and_no_host_sync():
    dev = _gpu()
    from bmc_hip.encodings import event_noise_mask
    H, W, n, dt = 180, 240, 100000, 2e-3
    cols, _, want = _case(H, W, n, dt, 2)
    xs, ys, ts, ps = (torch.tensor(c).to(dev) for c in cols)
    first = event_noise_mask(xs, ys, ts, (H, W), dt, 2)
    assert first.dtype == torch.uint8 and first.cpu().numpy().tobytes() == want.tobytes()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                               # the call itself waits for nothing
    try:
        keep, ps_out = event_noise_mask(xs, ys, ts, (H, W), dt, support=2, ps=ps)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        keep2, ps_out2 = event_noise_mask(xs, ys, ts, (H, W), dt, 2, ps)
    torch.cuda.synchronize()
    assert torch.equal(first, keep) and torch.equal(first, keep2)
    assert ps_out.cpu().numpy().tobytes() == ps_out2.cpu().numpy().tobytes() == np.where(want == 1, cols[3], 0.0).tobytes()
    assert torch.equal(ps, torch.tensor(cols[3]).to(dev))                 # the caller's column is not modified


# ------------------------------------------------------------------ 4. sessions
from test_gpu_multistream import SCALE, SEQN, _model  # noqa: E402

HF = dict(max_px=3, min_obvs=1, max_rate=0.6)
H_, W_ = 10, 16
GH, GW = SCALE * H_, SCALE * W_ - 2
NF_DT, PER_ITEM = 2e-2, 60


@functools.lru_cache(maxsize=None)
def _session_recordings():
    """Three event recordings of 6-7 windows, 60 LR events an item -> (lr columns, lr_index, gt columns, gt_index, ts, keep by the
    restatement for support 1 and 2)."""
    from test_gpu_event_slots import _columns
    out = []
    for k, nwin in enumerate([6, 7, 6]):
        rng = np.random.default_rng(700 + k)
        L = nwin + SEQN - 1
        xs, ys, ts, ps = R.stream(H_, W_, PER_ITEM * L, 0.3, seed=900 + nwin + k)
        ps[rng.choice(len(ps), 5, replace=False)] = 0.0                       # p == 0 is an event like any other
        lr_index = np.array([(PER_ITEM * j, PER_ITEM * (j + 1)) for j in range(L)], np.int64)
        gt = _columns(rng, 300 * L, GH, GW)
        gt_index = np.array([(300 * j, 300 * (j + 1)) for j in range(L)], np.int64)
        keep = {s: R.mask_seq(xs, ys, ts, H_, W_, NF_DT, s) for s in (1, 2)}
        assert all(0.05 <= v.mean() <= 0.95 for v in keep.values())
        out.append(((xs, ys, ps), lr_index, gt, gt_index, ts, keep))
    return out


def _dev(cols, dev):
    return tuple(torch.tensor(c).to(dev) for c in cols)


def _equal_entries(a, b):
    a, b = dict(a), dict(b)
    a.pop("time"), b.pop("time")
    assert set(a) == set(b) and len(a["esr_mse"]) > 0
    for key in a:
        if torch.is_tensor(a[key]):
            assert torch.equal(a[key], b[key]), key
        else:
            assert a[key] == b[key], key


@pytest.mark.parametrize("hot", [False, True], ids=["", "hot"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("plain", [False, True], ids=["full", "plain"])
def test_filtered_session_equals_prefiltered_columns(plain, graph, hot):
    """S = 2, three recordings: the first and the last opened with noise_filter (support 1 and 2), the middle one without -- against
    the session that is handed (xs, ys, ps * keep) with keep from the restatement: predictions and every entry of results()."""
    dev = _gpu()
    from bmc_hip import encodings
    from infer import MultiStreamSR
    n_c = 16
    m = _model(plain, n_c, seed=311).to(dev)
    recs = _session_recordings()
    support = [1, None, 2]
    kw = dict(n_c=n_c, scale=SCALE, plain=plain, graph=graph, keep_predictions=True, hot_filter=HF if hot else None)

    def run(filtered):
        ms = MultiStreamSR(m, 2, **kw)
        hs, held = [], []
        for (lr, li, gt, gi, ts, keep), s in zip(recs, support):
            cols = _dev(lr, dev)
            before, calls = cols[2].clone(), encodings.NOISE_CALLS
            if filtered and s is not None:
                nf = dict(ts=torch.tensor(ts).to(dev), dt=NF_DT, support=s)
                hs.append(ms.open_events(cols, _dev(gt, dev), li, gi, (H_, W_), (GH, GW), noise_filter=nf))
                assert encodings.NOISE_CALLS == calls + 1
            else:
                if s is not None:
                    cols = cols[:2] + (cols[2] * torch.tensor(keep[s]).to(dev),)
                hs.append(ms.open_events(cols, _dev(gt, dev), li, gi, (H_, W_), (GH, GW)))
                assert encodings.NOISE_CALLS == calls
            held.append((cols[2], before))
        calls = encodings.NOISE_CALLS
        ms.run()
        assert encodings.NOISE_CALLS == calls                                 # nothing enters a window
        if graph:
            assert ms._graph is not None and ms.replays > 0
        assert all(torch.equal(a, b) for (a, b), s in zip(held, support) if filtered)       # the caller's ps is not modified
        return [ms.results(h) for h in hs]

    got, want = run(True), run(False)
    for a, b, (lr, _, _, _, _, keep), s in zip(got, want, recs, support):
        a = dict(a)
        if s is None:
            assert "noise_events" not in a
        else:
            assert a.pop("noise_events") == len(keep[s]) - int(keep[s].sum()) > 0
        assert ("hot_pixels" in a) == hot
        _equal_entries(a, b)
    plainrun = MultiStreamSR(m, 2, **kw)                                      # the filter acted: unfiltered predictions differ
    lr, li, gt, gi, _, _ = recs[0]
    h = plainrun.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H_, W_), (GH, GW))
    plainrun.run()
    assert not torch.equal(plainrun.results(h)["predictions"], got[0]["predictions"])


def test_unfiltered_recordings_launch_what_they_did_and_refusals():
    """A session whose recordings are opened without the option: the launches per window of a session before the option existed
    (the accounting of test_gpu_hot_filter.py::test_launches_and_bytes), with a filtered recording beside them too."""
    dev = _gpu()
    from bmc_hip import encodings, slots
    from infer import MultiStreamSR
    n_c = 16
    m = _model(False, n_c, seed=313).to(dev)
    recs = _session_recordings()[:2]

    def session(filtered):
        ms = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE, keep_predictions=True)
        for k, (lr, li, gt, gi, ts, _) in enumerate(recs):
            nf = dict(ts=torch.tensor(ts).to(dev), dt=NF_DT) if k in filtered else None
            ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H_, W_), (GH, GW), noise_filter=nf)
        per = []
        while True:
            before = (dict(slots.LAUNCHES), slots.ENCODE_LAUNCHES, slots.HOT_LAUNCHES, encodings.NOISE_CALLS)
            if not ms.step():
                break
            per.append(({k: slots.LAUNCHES[k] - before[0][k] for k in before[0]}, slots.ENCODE_LAUNCHES - before[1],
                        slots.HOT_LAUNCHES - before[2], encodings.NOISE_CALLS - before[3]))
        return ms, per

    one = {"stage": 1, "commit": 1, "metrics": 1}
    (off, per0), (mixed, per1) = session(()), session((1,))
    assert per0 == per1 and all(p == (one, 1, 0, 0) for p in per0)
    assert off.scratch_bytes() == mixed.scratch_bytes()
    lr, li, gt, gi, ts, _ = recs[0]
    ms = MultiStreamSR(m, 2, n_c=n_c, scale=SCALE)
    t = torch.tensor(ts).to(dev)
    for nf, match in ((dict(ts=t), "lacks the key 'dt'"), (dict(ts=t, dt=NF_DT, k=2), "unknown key 'k'"), (dict(ts=t[:-1], dt=NF_DT), "ts has"),
                      (dict(ts=t.flip(0), dt=NF_DT), "finite and non-decreasing"), (dict(ts=t, dt=-1.0), "dt"), (dict(ts=t, dt=NF_DT, support=9), "support")):
        with pytest.raises(ValueError, match=match):
            ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H_, W_), (GH, GW), noise_filter=nf)
    assert not ms._recs                                                       # a refused recording is not queued


# ------------------------------------------------------------------ 5. the training set
@pytest.mark.parametrize("crop", [None, (6, 8)], ids=["full", "crop"])
def test_training_set_equals_prefiltered_columns(crop):
    dev = _gpu()
    import random
    from event_dataset import EventTrainSet
    recs = _session_recordings()

    def build(filtered):
        ts_ = EventTrainSet(L=4, step_size=2, crop=crop, scale=SCALE)
        for k, (lr, li, gt, gi, ts, keep) in enumerate(recs):
            cols = _dev(lr, dev)
            if k == 1:                                                        # the middle recording is not filtered
                r = ts_.add_recording(cols, _dev(gt, dev), li, gi, (H_, W_), (GH, GW))
                assert ts_.noise_dropped(r) is None
            elif filtered:
                before = cols[2].clone()
                r = ts_.add_recording(cols, _dev(gt, dev), li, gi, (H_, W_), (GH, GW),
                                      noise_filter=dict(ts=torch.tensor(ts).to(dev), dt=NF_DT, support=2))
                assert ts_.noise_dropped(r) == len(keep[2]) - int(keep[2].sum()) > 0 and torch.equal(cols[2], before)
            else:
                ts_.add_recording(cols[:2] + (cols[2] * torch.tensor(keep[2]).to(dev),), _dev(gt, dev), li, gi, (H_, W_), (GH, GW))
        return ts_

    a, b, raw = build(True), build(False), EventTrainSet(L=4, step_size=2, crop=crop, scale=SCALE)
    lr, li, gt, gi, _, _ = recs[0]
    raw.add_recording(_dev(lr, dev), _dev(gt, dev), li, gi, (H_, W_), (GH, GW))
    idx = list(range(len(a)))
    assert len(a) == len(b) >= 6
    (ia, ga), (ib, gb) = a.batch(idx, rng=random.Random(3)), b.batch(idx, rng=random.Random(3))
    assert torch.equal(ia, ib) and torch.equal(ga, gb) and ia.abs().sum() > 0
    ir, gr = raw.batch(idx[:2], rng=random.Random(3))
    assert not torch.equal(ir, ia[:2]) and torch.equal(gr, ga[:2])            # the filter acted, the ground truth is untouched
    with pytest.raises(ValueError, match="noise_filter has an unknown key"):
        a.add_recording(_dev(lr, dev), _dev(gt, dev), li, gi, (H_, W_), (GH, GW), noise_filter=dict(ts=None, dt=1.0, window=2))


# ------------------------------------------------------------------ 6. the tool
def test_tool_noise_filter_row_parses():
    _gpu()
    import json
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "multistream_infer.py"), "--noise-filter", "0.002:1", "--sizes", "31x56",
                        "--slots", "2", "--windows", "2", "--warmup", "3", "--modes", "graph", "--runs", "1"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    rows = [json.loads(ln) for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    row = next(r for r in rows if r.get("noise_filter"))
    assert row["events"] and row["noise_filter"] == {"dt": 0.002, "support": 1} and 0.15 < row["noise_share"] < 0.25
    assert 0.0 < row["dropped_share"] < 1.0 and row["esr_mse"] > 0 and row["esr_mse_filter_off"] > 0
    assert row["ms_per_window"] > 0 and row["ms_per_window_filter_off"] > 0
