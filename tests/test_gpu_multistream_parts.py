"""MultiStreamSR's options side by side (infer.py, infer_parts.py): a session with every option on gives, key by key and byte
for byte, what the sessions with one option on give (the single-option sessions are pinned to the reference's goldens by the
tests of each option); its byte counts are those of the buffers it allocates; a running session that grows rebuilds the
buffers of the part that grew and no others.

Every case: the 16-channel model, scale 4, 12 x 20 frames, 2 slots, three recordings of 3, 2 and 4 windows (the 4-window one
takes over the slot of the 2-window one) -- event-backed with ground truth, frame-backed with ground truth (and spans= in a
timed session), frame-backed without ground truth.  The ground truth is 40 x 72, not the prediction's 48 x 80, so the pictures
use the resized-esr table."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_event_slots import _dev, _recording
from test_gpu_multistream import SCALE, SEQN, _model, _recordings

pytestmark = pytest.mark.gpu
N_C, S, H, W, GH, GW = 16, 2, 12, 20, 40, 72
SH, SW = SCALE * H, SCALE * W
WINDOWS = (3, 2, 4)
PER_WINDOW = 16 * 2 * SH * SW                              # room for 16 events per element of a window
OPTIONS = {"keep": dict(keep_predictions=True), "stream": dict(emit_events=True, event_times="linear"),
           "hot": dict(hot_filter=dict(max_px=100, min_obvs=1, max_rate=0.5)),
           "render": dict(render=("lr", "bicubic", "esr", "gt")), "voxel": dict(voxel_bins=5)}
KEY_OPTION = {"esr_mse": "keep", "bicubic_mse": "keep", "predictions": "keep", "sr_events": "stream", "sr_index": "stream",
              "sr_ts": "stream", "hot_pixels": "hot", "hot_mask": "hot", "images": "render", "voxels": "voxel"}
# what scratch_bytes() counts; x, pred, pool, feat, table and emit_parts it does not
COUNTED = ("lr_scratch", "gt_scratch", "hot_counts", "hot_ring", "hot_ws", "emit_scratch", "render_minmax", "render_resize",
           "render_mid", "voxel_parts")
# per window: one call of each wrapper; one render call per table in use: lr, esr (no ground truth), esr_gt, bicubic, gt
LAUNCHES = dict(stage=1, commit=1, metrics=1, encode=1, hot=1, emit=0, timed=1, render=5, voxel=1)


@functools.lru_cache(maxsize=None)
def _case():
    (fb, gb), (fc, _) = _recordings(WINDOWS[1:], H, W, GH, GW, 4072)
    L = WINDOWS[1] + SEQN - 1
    t0 = 123456789.0 + 3048.0 * np.arange(L)
    return _recording(4071, WINDOWS[0], H, W, GH, GW), (fb, gb, np.stack([t0, t0 + 3048.0], 1)), fc


def _session(graph, names):
    from infer import MultiStreamSR
    kw = {}
    for n in names:
        kw.update(OPTIONS[n])
    return MultiStreamSR(_model(False, N_C, seed=4073).to(_gpu()), S, n_c=N_C, scale=SCALE, graph=graph, **kw)


def _open(ms):
    """The three recordings -> their handles."""
    dev = _gpu()
    (lr, gt, li, gi), (fb, gb, spans), fc = _case()
    room = dict(event_capacity=max(WINDOWS) * PER_WINDOW, window_event_capacity=PER_WINDOW) if ms.emit_events else {}
    return [ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (GH, GW), **room),
            ms.open(fb.to(dev), gb.to(dev), spans=spans if ms.event_times else None, **room), ms.open(fc.to(dev), **room)]


def _counters():
    from bmc_hip import slots
    return dict(slots.LAUNCHES, encode=slots.ENCODE_LAUNCHES, hot=slots.HOT_LAUNCHES, emit=slots.EMIT_LAUNCHES,
                timed=slots.EMIT_TIMED_LAUNCHES, render=slots.RENDER_LAUNCHES, voxel=slots.VOXEL_LAUNCHES)


def _step(ms):
    """One step -> how far every launch counter moved (None: nothing was left to run)."""
    before = _counters()
    if not ms.step():
        return None
    return {k: v - before[k] for k, v in _counters().items()}


@functools.lru_cache(maxsize=None)
def _run(graph, *names):
    """The session with the options `names` on the three recordings -> (results per recording, counter moves per step, replays)."""
    ms = _session(graph, names)
    hs = _open(ms)
    per = list(iter(lambda: _step(ms), None))
    torch.cuda.synchronize()
    return [ms.results(h) for h in hs], per, ms.replays


def _equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return set(a) == set(b) and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return isinstance(a, list) and a == b


# ------------------------------------------------------------------ 1. all options compose
@pytest.mark.parametrize("graph", [False, True])
def test_all_options_compose(graph):
    """Every key of every recording equals the key of the eager session with only that key's option on.  The hot-pixel filter
    changes what the model sees of the event-backed recording 0, so for that recording the session with one option on has the
    filter on beside it (hot_pixels and hot_mask come from the session with the filter alone)."""
    res, per, replays = _run(graph, *OPTIONS)
    for k, r in enumerate(res):
        want = set(KEY_OPTION) - ({"hot_pixels", "hot_mask"} if k else set()) - ({"esr_mse", "bicubic_mse"} if k == 2 else set())
        assert set(r) == want | {"time"} and len(r["time"]) == WINDOWS[k]
        assert set(r["images"]) == ({"lr", "esr"} if k == 2 else set(OPTIONS["render"]["render"]))
        assert r["sr_ts"].dtype == (torch.float64 if k == 1 else torch.float32) and r["sr_ts"].numel() == int(r["sr_index"][-1]) > 0
        for key in sorted(want):
            option = KEY_OPTION[key]
            single = _run(False, option, "hot") if k == 0 and option != "hot" else _run(False, option)
            assert _equal(r[key], single[0][k][key]), (k, key)
    assert res[0]["hot_mask"].min() == 0                               # the filter did mask
    assert len(per) == 6
    if graph:                                                          # two eager windows, the capture, then replays only
        assert per[:3] == [LAUNCHES] * 3 and per[3:] == [dict.fromkeys(LAUNCHES, 0)] * 3 and replays == 4
    else:
        assert per == [LAUNCHES] * 6 and replays == 0


# ------------------------------------------------------------------ 2. byte counts
def _reachable(v):
    if torch.is_tensor(v):
        return [v]
    if isinstance(v, dict):
        v = list(v.values())
    return [t for x in v for t in _reachable(x)] if isinstance(v, (tuple, list)) else []


@functools.lru_cache(maxsize=None)
def _bytes(names):
    ms = _session(False, names)
    hs = _open(ms)
    before = ms.scratch_bytes()
    assert ms._bufs is None and ms.step()
    b = ms._bufs
    resident = [(ms.resident_bytes(h), sum(t.numel() * t.element_size() for t in _reachable(ms._recs[h]))) for h in hs]
    return before, ms.scratch_bytes(), sum(b[k].numel() * b[k].element_size() for k in COUNTED if k in b), sorted(b), resident


@pytest.mark.parametrize("names", [(), ("render",), ("stream",), ("render", "stream"), tuple(OPTIONS)], ids=lambda n: "+".join(n) or "none")
def test_byte_counts(names):
    """scratch_bytes() before the first step = after it = the bytes of the counted buffers the session holds.  With render and
    event_times on it is the two single-option values together -- each over the value with no option on, which is the scratch
    of the event-backed recording's slots that all of them hold.  resident_bytes() = every tensor of the record."""
    before, after, held, keys, resident = _bytes(names)
    print(names, before, after, held, keys)
    assert before == after == held > 0
    assert ("emit_parts" in keys) == ("stream" in names) and {"lr_scratch", "gt_scratch"} <= set(keys)
    if names == ("render", "stream"):
        none, render, stream = (_bytes(n)[0] for n in ((), ("render",), ("stream",)))
        assert render > none and stream > none and before - none == (render - none) + (stream - none)
    assert all(got == want > 0 for got, want in resident)


# ------------------------------------------------------------------ 3. growth
def test_a_running_session_rebuilds_only_what_grew():
    """Graph mode, every option on, three windows on frame-backed recordings; then the first event-backed recording, the first
    clocked one and one with a larger window_event_capacity are opened: each drops the graph and rebuilds exactly the buffers of
    the part that grew (the table where a keyword changed), and the next step captures once."""
    dev = _gpu()
    ms = _session(True, tuple(OPTIONS))
    (lr, gt, li, gi), (fb, gb, spans), _ = _case()
    (f0, g0), (f1, g1) = _recordings((4, 14), H, W, GH, GW, 4074)
    room = dict(event_capacity=14 * PER_WINDOW, window_event_capacity=PER_WINDOW)
    hs = [ms.open(f0.to(dev), g0.to(dev), **room), ms.open(f1.to(dev), g1.to(dev), **room)]
    assert [_step(ms) for _ in range(3)] == [LAUNCHES | dict(encode=0, hot=0)] * 3 and ms._graph is not None
    grown = [(lambda: ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (GH, GW), **room),
              {"table", "lr_scratch", "gt_scratch", "hot_counts", "hot_ring", "hot_ws"}),
             (lambda: ms.open(fb.to(dev), gb.to(dev), spans=spans, **room), {"table"}),
             (lambda: ms.open(fb.to(dev), gb.to(dev), **dict(room, window_event_capacity=2 * PER_WINDOW)), {"emit_scratch"})]
    for open_, rebuilt in grown:
        held = dict(ms._bufs)
        hs.append(open_())
        assert ms._graph is None
        assert {k for k, t in ms._bufs.items() if t is not held.get(k)} == rebuilt
        assert _step(ms) == LAUNCHES and ms._graph is not None            # the capture
        assert _step(ms) == dict.fromkeys(LAUNCHES, 0)                                     # a replay
    assert ms._has_clock and ms._wcap == 2 * PER_WINDOW
    ms.run()
    torch.cuda.synchronize()
    for h, n in zip(hs, (4, 14, WINDOWS[0], WINDOWS[1], WINDOWS[1])):
        r = ms.results(h)
        assert len(r["time"]) == n == len(r["predictions"]) == len(r["voxels"]) == len(r["sr_index"]) - 1
