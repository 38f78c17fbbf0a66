"""The integrate-and-fire event downsampler on the GPU: the entry points of include/bmc_hip_downsample.h byte for byte -- keys, all
four output columns and count -- against the sequential restatement (tests/event_downsample_ref.py::downsample_seq), outputs
pre-filled inside guard regions, inputs and guards checked untouched; downsample_events; add_hr_recording and open_hr_events
against add_recording / open_events on the restatement's LR columns; the launch accounting."""
import functools
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import event_downsample_ref as R
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
NAN = float("nan")


def _guarded(n, dtype, fill, dev):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _prefilled(t, fill):
    return bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())


def _same(a, b):
    """torch.equal on the bits: a NaN polarity equals itself."""
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _call(dev, cols, H, W, s, T):
    """keys, the grouping sort, walk and gather on numpy columns, every buffer the library writes pre-filled inside guard regions
    -> (keys, fire, (xs, ys, ts, ps) at full capacity, count, capacity) as numpy / int.  The guards, the input columns and the
    sorted keys and permutation are checked untouched."""
    from bmc_hip import downsample_lib as D, lib, ops
    xs, ys, ts, ps = (torch.tensor(c).to(dev) for c in cols)
    before = [t.clone() for t in (xs, ys, ts, ps)]
    n, st = xs.numel(), ops._stream()
    cap = D.capacity(n, T)
    assert cap == n // T
    fills = dict(keys=(torch.int32, -7), fire=(torch.int8, 0x55), oxs=(torch.int16, -3), oys=(torch.int16, -3), ots=(torch.float64, NAN),
                 ops=(torch.float64, NAN), count=(torch.int64, -1), scratch=(torch.int64, -1))
    sizes = dict(keys=n, fire=n, oxs=cap, oys=cap, ots=cap, ops=cap, count=1, scratch=D.scratch_bytes(n) // 8)
    bufs = {k: _guarded(sizes[k], *fills[k], dev) for k in fills}
    v = {k: b[1] for k, b in bufs.items()}
    ptr = lambda t: t.data_ptr() if t.numel() else None
    lib.call(D._keys, "keys", ptr(xs), ptr(ys), ptr(ps), n, H, W, s, ptr(v["keys"]), ptr(v["fire"]), st)
    keys = v["keys"].cpu().numpy().copy()
    assert bool((v["fire"] == 0).all())                                        # the keys launch is the zero fill
    if n:
        skeys, perm = torch.sort(v["keys"], stable=True)
        held = skeys.clone(), perm.clone()
        lib.call(D._walk, "walk", skeys.data_ptr(), perm.data_ptr(), ps.data_ptr(), n, H, W, s, T, v["fire"].data_ptr(), st)
    lib.call(D._gather, "gather", ptr(xs), ptr(ys), ptr(ts), ptr(v["fire"]), n, s, ptr(v["oxs"]), ptr(v["oys"]), ptr(v["ots"]),
             ptr(v["ops"]), cap, v["count"].data_ptr(), v["scratch"].data_ptr(), st)
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        edge = torch.cat([buf[:GUARD], buf[-GUARD:]])
        assert _prefilled(edge, fills[k][1]), k
    assert all(_same(a, b) for a, b in zip(before, (xs, ys, ts, ps)))
    assert not n or (torch.equal(held[0], skeys) and torch.equal(held[1], perm) and torch.equal(v["keys"], torch.tensor(keys).to(dev)))
    out = tuple(v[k].cpu().numpy() for k in ("oxs", "oys", "ots", "ops"))
    return keys, v["fire"].cpu().numpy(), out, int(v["count"][0]), cap


def _agrees(dev, cols, H, W, s, T, want=None):
    """The entry points against the restatement: keys, count, the head of every column byte for byte, the tail as pre-filled."""
    xs, ys, ts, ps = cols
    if want is None:
        want = R.downsample_seq(xs, ys, ts, ps, H, W, s, T)
    h, w = R.lr_size(H, W, s)
    keys, fire, out, count, cap = _call(dev, cols, H, W, s, T)
    ok = R.counted(xs, ys, ps, H, W)
    want_keys = np.where(ok, (ys.astype(np.int64) // s) * w + xs.astype(np.int64) // s, h * w).astype(np.int32)
    assert keys.tobytes() == want_keys.tobytes()
    k = len(want[0])
    assert count == k <= cap and int((fire != 0).sum()) == k and set(np.unique(fire).tolist()) <= {-1, 0, 1}
    for name, got, ref, fill in zip(("xs", "ys", "ts", "ps"), out, want[:4], (-3, -3, NAN, NAN)):
        assert got.dtype == ref.dtype and got[:k].tobytes() == ref.tobytes(), (name, H, W, s, T, len(xs))
        assert _prefilled(torch.tensor(got[k:]), fill), name                  # nothing at count and after
    return want


# ------------------------------------------------------------------ 1. the entry points, byte for byte
SHAPES = [(1, 1, 1, 300), (2, 2, 2, 300), (5, 7, 2, 700), (8, 12, 4, 2000), (37, 53, 4, 6000), (37, 53, 3, 6000), (180, 240, 4, 160000),
          (64, 96, 1, 9000), (70, 90, 2, 9000)]


@functools.lru_cache(maxsize=None)
def _case(H, W, s, n, T, seed=0):
    cols = R.stream(H, W, n, s, seed=H * W + n + s + seed)
    return cols, R.downsample_seq(*cols, H, W, s, T)


@pytest.mark.parametrize("T", [1, "s*s", 32767])
@pytest.mark.parametrize("H,W,s,n", SHAPES, ids=lambda v: str(v))
def test_entry_points_equal_the_restatement(H, W, s, n, T):
    dev = _gpu()
    from bmc_hip import downsample_lib as D
    T = s * s if T == "s*s" else T
    h, w = R.lr_size(H, W, s)
    if (H, W) in ((180, 240), (64, 96), (70, 90)):
        assert h * w > 4 * D.LANES                                             # several walk workgroups
    if (H, W, s) in ((5, 7, 2), (37, 53, 4), (37, 53, 3)):
        assert H % s and W % s                                                 # ragged edge blocks
    cols, want = _case(H, W, s, n, T)
    k = len(want[0])
    print("%d LR events of %d HR events, capacity %d" % (k, n, n // T))
    if T <= s * s and H * W > 1:
        assert k > n // (8 * T) and {-1.0, 1.0} == set(want[3].tolist())       # it fires, both ways
    if T == 32767:
        assert k == 0                                                          # a stream with no output
    _agrees(dev, cols, H, W, s, T, want)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1023, 1024, 1025, 5000])
def test_stream_lengths_around_a_workgroup_and_a_gather_chunk(n):
    dev = _gpu()
    from bmc_hip import downsample_lib as D
    assert D.LANES == 256 and D.chunk(n) == D.TILE == 1024 and (n != 5000 or D.scratch_bytes(n) == 8 * 3)      # 5000: five chunks
    for H, W, s, T in ((5, 7, 2, 1), (5, 7, 2, 4), (8, 12, 4, 2)):
        cols, want = _case(H, W, s, n, T, seed=1)
        assert n < 255 or len(want[0]) > 0
        _agrees(dev, cols, H, W, s, T, want)


# ------------------------------------------------------------------ 2. planted streams
def test_one_long_segment_and_one_block():
    dev = _gpu()
    H, W, s, T, n = 37, 53, 4, 16, 5000
    rng = np.random.default_rng(5)
    ps = np.where(rng.random(n) < 0.9, 1.0, -1.0) * np.where(np.arange(n) < n // 2, 1.0, -1.0)
    ts = np.sort(np.round(rng.random(n) * 1e6) / 1e6)
    one = (np.full(n, 21, np.int16), np.full(n, 9, np.int16), ts, ps)          # every event on one HR pixel
    want = _agrees(dev, one, H, W, s, T)
    assert len(want[0]) > 200 and {-1.0, 1.0} == set(want[3].tolist()) and set(want[0].tolist()) == {5} and set(want[1].tolist()) == {2}
    block = ((20 + rng.integers(0, 4, n)).astype(np.int16), (8 + rng.integers(0, 4, n)).astype(np.int16), ts, ps)     # ... in one LR block
    assert len(set(zip(block[0].tolist(), block[1].tolist()))) == 16
    got = _agrees(dev, block, H, W, s, T)
    assert R.same(got[:4], want[:4])                                           # the block adds its pixels: the same LR stream
    edge = ((52 + 0 * rng.integers(0, 4, n)).astype(np.int16), (36 + 0 * rng.integers(0, 4, n)).astype(np.int16), ts, ps)
    got = _agrees(dev, edge, H, W, s, T)                                       # the corner block is one HR pixel and keeps T
    assert len(got[0]) == len(want[0]) and set(got[0].tolist()) == {13} and set(got[1].tolist()) == {9}


def test_capacity_filled_exactly_and_no_output():
    dev = _gpu()
    for T, k, sign in ((1, 1300, 1.0), (16, 130, -1.0), (32767, 2, 1.0)):
        n = k * T
        cols = R.columns([5] * n, [6] * n, [sign] * n)
        want = _agrees(dev, cols, 8, 12, 4, T)
        assert len(want[0]) == k == n // T and (want[3] == sign).all()         # reached: the columns are full
        want = _agrees(dev, tuple(c[:-1] for c in cols), 8, 12, 4, T)
        assert len(want[0]) == k - 1 == (n - 1) // T
    n = 3000
    xs, ys, ps = R.alternating(n, 5, 6)
    assert len(_agrees(dev, R.columns(xs, ys, ps), 8, 12, 4, 2)[0]) == 0       # alternating signs never fire
    zeros = R.columns(xs, ys, [0.0, -0.0, NAN] * (n // 3))
    assert len(_agrees(dev, zeros, 8, 12, 4, 1)[0]) == 0                       # nothing is counted
    out = R.columns([-1, 12, 3, 3] * (n // 4), [2, 2, -1, 8] * (n // 4), [1.0] * n)
    assert len(_agrees(dev, out, 8, 12, 4, 1)[0]) == 0                         # everything is out of range


@pytest.mark.parametrize("T", [2, 6])
def test_hysteresis_across_workgroup_and_chunk_boundaries(T):
    """The hysteresis plants placed so that a pixel's events -- and the firing event itself -- sit on both sides of index 256 (two
    keys workgroups) and of index 1024 (two gather chunks); the rest of the stream alternates on another pixel and never fires."""
    dev = _gpu()
    H, W, s, n = 8, 12, 4, 1300
    for edge in (256, 1024):
        for fire_at in (edge - 1, edge):
            xs, ys, ps = [9] * n, [1] * n, [None] * n
            px, py, pp = R.exact_fire(T, 2, 5)                                  # fires at its event T-1, then T-1 more: no second fire
            a = fire_at - (T - 1)
            xs[a:a + len(pp)], ys[a:a + len(pp)], ps[a:a + len(pp)] = px, py, pp
            hx, hy, hp = R.hysteresis_no_fire(T, 6, 2)                          # T-1 ups, one down, one up: across the other edge
            b = (1280 - edge) - T // 2
            xs[b:b + len(hp)], ys[b:b + len(hp)], ps[b:b + len(hp)] = hx, hy, hp
            filler = [i for i in range(n) if ps[i] is None]                    # the rest alternates among itself on pixel (9, 1)
            for j, i in enumerate(filler):
                ps[i] = 1.0 if j % 2 == 0 else -1.0
            want = _agrees(dev, R.columns(xs, ys, ps), H, W, s, T)
            assert want[2].tolist() == [fire_at * 1e-6] and want[0].tolist() == [0] and want[1].tolist() == [1] and want[3].tolist() == [1.0]
            assert want[4][1, 0] == T - 1 and want[4][0, 1] == T - 1


def test_a_polarity_column_from_the_noise_filter():
    dev = _gpu()
    from bmc_hip.encodings import downsample_events, event_noise_mask
    H, W, s, n = 37, 53, 4, 6000
    xs, ys, ts, ps = R.stream(H, W, n, s, seed=11, nan=False)
    d = [torch.tensor(c).to(dev) for c in (xs, ys, ts, ps)]
    keep, ps_out = event_noise_mask(d[0], d[1], d[2], (H, W), 5e-3, 1, ps=d[3])
    dropped = ps_out.cpu().numpy()
    assert 0.05 < float(keep.float().mean()) < 0.95 and int((dropped == 0).sum()) > n // 20      # zeros present
    for T in (4, 16):
        want = _agrees(dev, (xs, ys, ts, dropped), H, W, s, T)
        raw = R.downsample_seq(xs, ys, ts, ps, H, W, s, T)
        assert 0 < len(want[0]) < len(raw[0])                                  # the dropped events touched nothing
    got = downsample_events(d[0], d[1], d[2], ps_out, (H, W), s)
    assert R.same(tuple(t.cpu().numpy() for t in got[:4]), want[:4]) and got[4] == (10, 14)


# ------------------------------------------------------------------ 3. downsample_events
def test_downsample_events_trim_count_same_bytes_and_no_host_sync():
    dev = _gpu()
    from bmc_hip import downsample_lib as D, encodings
    from bmc_hip.encodings import downsample_events
    H, W, s, n = 180, 240, 4, 160000
    cols, want = _case(H, W, s, n, 16)
    d = [torch.tensor(c).to(dev) for c in cols]
    calls, launches = encodings.DOWNSAMPLE_CALLS, encodings.DOWNSAMPLE_LAUNCHES
    first = downsample_events(*d, (H, W), s)                                   # threshold None = s * s
    assert (encodings.DOWNSAMPLE_CALLS, encodings.DOWNSAMPLE_LAUNCHES) == (calls + 1, launches + D.LAUNCHES) and D.LAUNCHES == 4
    assert len(first) == 5 and first[4] == (45, 60) and [t.dtype for t in first[:4]] == [torch.int16, torch.int16, torch.float64, torch.float64]
    assert all(t.is_contiguous() and t.device == d[0].device for t in first[:4])
    assert R.same(tuple(t.cpu().numpy() for t in first[:4]), want[:4]) and len(want[0]) > 1000
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                    # trim=False waits for nothing
    try:
        second = downsample_events(*d, (H, W), s, 16, trim=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = downsample_events(*d, (H, W), s, threshold=16, trim=False)
    torch.cuda.synchronize()
    k = len(want[0])
    for run in (second, third):
        assert len(run) == 6 and run[4] == (45, 60) and run[5].dtype == torch.int64 and run[5].tolist() == [k]
        assert all(t.numel() == n // 16 for t in run[:4])                      # the capacity
        assert all(torch.equal(a, b[:k]) for a, b in zip(first[:4], run[:4]))  # identical bytes run after run
    assert all(_same(a, torch.tensor(c).to(dev)) for a, c in zip(d, cols))                       # the caller's columns
    empty = downsample_events(*(t[:0] for t in d), (H, W), s)
    assert all(t.numel() == 0 for t in empty[:4]) and encodings.DOWNSAMPLE_LAUNCHES == launches + 3 * D.LAUNCHES + 2
    one = downsample_events(*(t[:5] for t in d), (H, W), s)                    # fewer events than T: capacity 0
    assert all(t.numel() == 0 for t in one[:4])
    with pytest.raises(ValueError, match="^downsample_events: .*one device"):
        downsample_events(d[0], d[1], d[2].cpu(), d[3], (H, W), s)


def test_entry_point_refusals_and_the_empty_stream():
    dev = _gpu()
    from bmc_hip import downsample_lib as D, lib
    buf = torch.full((64,), -1, dtype=torch.int64, device=dev)
    p = buf.data_ptr()
    assert D._keys(None, None, None, 0, 5, 7, 2, None, None, None) == 0 and D._walk(None, None, None, 0, 5, 7, 2, 4, None, None) == 0
    assert D._gather(None, None, None, None, 0, 2, None, None, None, None, 0, p, p + 8, None) == 0
    torch.cuda.synchronize()
    assert buf[0].item() == 0 and bool((buf[2:] == -1).all())                   # n == 0 writes count = 0 (and one chunk total)
    for kw in (dict(n=1 << 31), dict(s=17), dict(cap=-1), dict(count=None), dict(scratch=p + 4), dict(fire=None), dict(ops=None)):
        good = dict(xs=p, ys=p, ts=p, fire=p, n=4, s=2, oxs=p, oys=p, ots=p, ops=p, cap=1, count=p, scratch=p, st=None)
        assert D._gather(*{**good, **kw}.values()) == -1 and b"bmc_event_downsample_gather" in lib.bmc_last_error(), kw
    torch.cuda.synchronize()
    assert buf[0].item() == 0 and bool((buf[2:] == -1).all())                   # refused before any launch


# ------------------------------------------------------------------ 4. sessions and the training set
from test_gpu_multistream import SCALE, SEQN, _model  # noqa: E402

GH, GW = 40, 62                                              # -> 10 x 16: the last LR column covers two HR columns
LH, LW = 10, 16
WINDOW, SLIDING, N_HR = 120, 60, 24000
NF = dict(dt=2e-2, support=1)


@functools.lru_cache(maxsize=None)
def _hr_recordings():
    """Three HR-only recordings of 6-7 windows -> (gt columns, gt_ts, L, the restatement's LR columns and lr_ts, both index
    tables of event_window_indices on them)."""
    from bmc_hip.encodings import event_window_indices
    out = []
    for k, nwin in enumerate([6, 7, 6]):
        L = nwin + SEQN - 1
        xs, ys, ts, ps = R.stream(GH, GW, N_HR, SCALE, seed=40 + k, nan=False)
        lx, ly, lt, lp, _ = R.downsample_seq(xs, ys, ts, ps, GH, GW, SCALE, SCALE * SCALE)
        assert len(lx) >= (WINDOW - SLIDING) * (L + 1) and lx.max() == LW - 1 and ly.max() == LH - 1
        li, gi = event_window_indices(lt, ts, WINDOW, SLIDING, SCALE, L)
        assert len(li) == len(gi) == L
        out.append(((xs, ys, ps), ts, L, (lx, ly, lp), lt, li, gi))
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
        elif isinstance(a[key], (tuple, list)) and any(torch.is_tensor(v) for v in a[key]):
            assert len(a[key]) == len(b[key]) and all(torch.equal(u, v) for u, v in zip(a[key], b[key])), key
        else:
            assert a[key] == b[key], key


@pytest.mark.parametrize("mode", ["eager", "graph", "timed", "filtered"])
def test_hr_session_equals_open_events_on_the_restatements_columns(mode):
    """S = 2, three HR-only recordings through open_hr_events against the session that is handed the restatement's LR columns and
    the same tables: predictions and every entry of results().  timed: an event_times session, which gets the synthesized lr_ts;
    filtered: noise_filter without ts.  One downsampling per recording at the door, nothing per window."""
    dev = _gpu()
    from bmc_hip import downsample_lib as D, encodings, slots
    from infer import MultiStreamSR
    n_c = 16
    m = _model(False, n_c, seed=411).to(dev)
    recs = _hr_recordings()
    kw = dict(n_c=n_c, scale=SCALE, graph=mode == "graph", keep_predictions=True)
    if mode == "timed":
        kw.update(emit_events=True, event_times="linear")

    def run(from_hr):
        ms = MultiStreamSR(m, 2, **kw)
        hs = []
        for gt, gt_ts, L, lr, lt, li, gi in recs:
            g, t = _dev(gt, dev), torch.tensor(gt_ts).to(dev)
            held = [c.clone() for c in g + (t,)]
            before = encodings.DOWNSAMPLE_CALLS, encodings.DOWNSAMPLE_LAUNCHES
            if from_hr:
                hs.append(ms.open_hr_events(g, t, (GH, GW), window=WINDOW, sliding_window=SLIDING, dataset_length=L,
                                            noise_filter=NF if mode == "filtered" else None))
                assert (encodings.DOWNSAMPLE_CALLS, encodings.DOWNSAMPLE_LAUNCHES) == (before[0] + 1, before[1] + D.LAUNCHES)
            else:
                lts = torch.tensor(lt).to(dev)
                hs.append(ms.open_events(_dev(lr, dev), g, li, gi, (LH, LW), (GH, GW), lr_ts=lts if mode == "timed" else None,
                                         noise_filter=dict(NF, ts=lts) if mode == "filtered" else None))
                assert (encodings.DOWNSAMPLE_CALLS, encodings.DOWNSAMPLE_LAUNCHES) == before
            assert all(torch.equal(a, b) for a, b in zip(held, g + (t,)))     # the caller's tensors are not modified
        per = []
        while True:
            before = dict(slots.LAUNCHES), slots.ENCODE_LAUNCHES, encodings.DOWNSAMPLE_CALLS, encodings.DOWNSAMPLE_LAUNCHES
            if not ms.step():
                break
            per.append(({k: slots.LAUNCHES[k] - before[0][k] for k in before[0]}, slots.ENCODE_LAUNCHES - before[1],
                        encodings.DOWNSAMPLE_CALLS - before[2], encodings.DOWNSAMPLE_LAUNCHES - before[3]))
        if mode == "graph":
            assert ms._graph is not None and ms.replays > 0
        return [ms.results(h) for h in hs], per, ms.scratch_bytes()

    (got, per_hr, bytes_hr), (want, per_lr, bytes_lr) = run(True), run(False)
    assert per_hr == per_lr and all(p[2:] == (0, 0) for p in per_hr) and bytes_hr == bytes_lr          # no launch enters a window
    if mode in ("eager", "filtered"):
        assert all(p[:2] == ({"stage": 1, "commit": 1, "metrics": 1}, 1) for p in per_hr)
    for a, b, rec in zip(got, want, recs):
        a = dict(a)
        assert a.pop("synthesized_events") == len(rec[3][0]) and "synthesized_events" not in b
        assert ("noise_events" in a) == (mode == "filtered") and (mode != "filtered" or a["noise_events"] > 0)
        assert ("sr_ts" in a) == (mode == "timed")
        _equal_entries(a, b)
        assert a["predictions"].abs().sum() > 0


def test_evaluate_recordings_takes_hr_only_recordings():
    dev = _gpu()
    from infer import EventRecording, HREventRecording, evaluate_recordings
    n_c = 16
    m = _model(False, n_c, seed=413).to(dev)
    gt, gt_ts, L, lr, lt, li, gi = _hr_recordings()[0]
    g, t = _dev(gt, dev), torch.tensor(gt_ts).to(dev)
    kw = dict(n_c=n_c, scale=SCALE, quality=True)
    # (the tables of the HR-only item are not capped by dataset_length: hand open_events the uncapped ones)
    from bmc_hip.encodings import event_window_indices
    li, gi = event_window_indices(lt, gt_ts, WINDOW, SLIDING, SCALE)
    a = evaluate_recordings(m, {"r": HREventRecording(g, t, (GH, GW), WINDOW, SLIDING)}, 1, **kw)
    b = evaluate_recordings(m, {"r": EventRecording(_dev(lr, dev), g, li, gi, (LH, LW), (GH, GW))}, 1, **kw)
    for k in ("esr_mse", "bicubic_mse", "esr_psnr", "esr_ssim", "bicubic_psnr", "bicubic_ssim"):
        assert np.array_equal(a["results"][k]["r"], b["results"][k]["r"], equal_nan=True), k
    assert a["results"]["esr_mse"]["r"] > 0 and np.isfinite(a["results"]["esr_psnr"]["r"])
    with pytest.raises(ValueError, match="gt_size .* differs"):
        evaluate_recordings(m, [HREventRecording(g, t, (GH, GW), WINDOW, SLIDING)], 1, gt_size=(GH, GW + 1), **kw)


@pytest.mark.parametrize("noise", [False, True], ids=["", "filtered"])
@pytest.mark.parametrize("crop", [None, (6, 8)], ids=["full", "crop"])
def test_training_set_equals_the_restatements_columns(crop, noise):
    dev = _gpu()
    from bmc_hip import downsample_lib as D, encodings
    from event_dataset import EventTrainSet
    recs = _hr_recordings()

    def build(from_hr):
        ts_ = EventTrainSet(L=4, step_size=2, crop=crop, scale=SCALE)
        for gt, gt_ts, L, lr, lt, li, gi in recs:
            g, t = _dev(gt, dev), torch.tensor(gt_ts).to(dev)
            held = [c.clone() for c in g + (t,)]
            before = encodings.DOWNSAMPLE_CALLS, encodings.DOWNSAMPLE_LAUNCHES
            if from_hr:
                r = ts_.add_hr_recording(g, t, (GH, GW), window=WINDOW, sliding_window=SLIDING, dataset_length=L,
                                         noise_filter=NF if noise else None)
                assert ts_.synthesized_events(r) == len(lr[0])
                assert (encodings.DOWNSAMPLE_CALLS, encodings.DOWNSAMPLE_LAUNCHES) == (before[0] + 1, before[1] + D.LAUNCHES)
            else:
                r = ts_.add_recording(_dev(lr, dev), g, li, gi, (LH, LW), (GH, GW),
                                      noise_filter=dict(NF, ts=torch.tensor(lt).to(dev)) if noise else None)
                assert ts_.synthesized_events(r) is None
            assert (ts_.noise_dropped(r) is not None) == noise and (not noise or ts_.noise_dropped(r) > 0)
            assert all(torch.equal(a, b) for a, b in zip(held, g + (t,)))
        return ts_

    a, b = build(True), build(False)
    assert [a.noise_dropped(r) for r in range(3)] == [b.noise_dropped(r) for r in range(3)]
    idx = list(range(len(a)))
    assert len(a) == len(b) >= 6
    before = encodings.DOWNSAMPLE_CALLS, encodings.DOWNSAMPLE_LAUNCHES
    (ia, ga), (ib, gb) = a.batch(idx, rng=random.Random(3)), b.batch(idx, rng=random.Random(3))
    assert (encodings.DOWNSAMPLE_CALLS, encodings.DOWNSAMPLE_LAUNCHES) == before                  # nothing enters a batch
    assert torch.equal(ia, ib) and torch.equal(ga, gb) and ia.abs().sum() > 0 and ga.abs().sum() > 0


def test_hr_entry_points_refuse():
    dev = _gpu()
    from event_dataset import EventTrainSet
    from infer import MultiStreamSR
    gt, gt_ts, L, *_ = _hr_recordings()[0]
    g, t = _dev(gt, dev), torch.tensor(gt_ts).to(dev)
    ms = MultiStreamSR(_model(False, 16, seed=415).to(dev), 2, n_c=16, scale=SCALE)
    ds = EventTrainSet(L=4, scale=SCALE)
    for who, call in (("MultiStreamSR.open_hr_events: ", ms.open_hr_events), ("EventTrainSet.add_hr_recording: ", ds.add_hr_recording)):
        for args, kw, match in (((g, t[:-1], (GH, GW)), {}, "ts has"), ((g, t, (GH, 0)), {}, "must be positive"),
                                ((g, t, (GH, GW)), dict(threshold=0), "threshold must be"),
                                ((g, t, (GH, GW)), dict(noise_filter=dict(ts=t, dt=1.0)), "keys dt, support"),
                                ((g, t, (GH, GW)), dict(noise_filter=dict(dt=-1.0)), r"noise_filter\['dt'\]"),
                                ((g, t, (GH, GW)), dict(noise_filter=dict(support=2)), "keys dt, support"),
                                ((g, t, (GH, GW)), dict(threshold=N_HR), "synthesized LR events"),     # one LR event at most: no block
                                ((g[:2], t, (GH, GW)), {}, "gt must be three tensors")):
            with pytest.raises(ValueError, match="^" + who.replace(".", r"\.") + ".*" + match):
                call(*args, **kw)
    assert not ms._recs and len(ds) == 0                                       # a refused recording is not queued


# ------------------------------------------------------------------ 5. the tool
def test_tool_from_hr_row_parses():
    _gpu()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "multistream_infer.py"), "--from-hr", "--sizes", "31x56",
                        "--slots", "2", "--windows", "2", "--warmup", "1", "--modes", "eager"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    rows = [json.loads(ln) for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    row = next(r for r in rows if r.get("runner") == "MultiStreamSR(events, from HR)")
    assert row["events"] and row["threshold"] == 16 and 0.05 < row["lr_events_per_hr_event"] <= 1 / 16
    assert row["ms_per_window"] > 0 and row["open_hr_events_ms"] > 0 and row["esr_mse"] > 0 and np.isfinite(row["esr_psnr"])
