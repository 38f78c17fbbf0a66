"""Event-count images on the GPU (include/bmc_hip.h, "event-count images"): bmc_slot_render through the plain-tensor entry
against the arrays the reference's plot_event_cnt returned and against the numpy restatement (tests/event_render_ref.py), and
MultiStreamSR(render=...) against the restatement applied to the tensors the session itself exposes -- all byte for byte."""
import functools

import numpy as np
import pytest
import torch

import event_render_ref as R
from test_event_render_cpu import golden_cases
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401
from test_gpu_multistream import SCALE, SEQN, _model, _recordings

pytestmark = pytest.mark.gpu
GUARD = 64
N_C = 16
ALL = ("lr", "bicubic", "esr", "gt")


def _np(t):
    return t.detach().cpu().numpy()


def _same(img, cnt, round=False, what=None):
    """img (uint8 GPU tensor [h,w,3]) is the restatement's picture of cnt (float32 tensor [2,h,w])."""
    want = R.render_np(_np(cnt), round=round)
    assert tuple(img.shape) == want.shape and img.dtype == torch.uint8, what
    assert _np(img).tobytes() == want.tobytes(), what


# ------------------------------------------------------------------ (a) the plain-tensor entry
def test_render_event_counts_equals_the_reference_and_the_restatement():
    dev = _gpu()
    from bmc_hip.encodings import render_event_counts
    n = 0
    for name, cnt, rnd, img in golden_cases():
        out = render_event_counts(torch.tensor(cnt)[None].to(dev), round=rnd)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (1,) + img.shape
        assert _np(out[0]).tobytes() == img.tobytes(), name
        assert _np(out[0]).tobytes() == R.render_np(cnt, round=rnd).tobytes(), name
        n += 1
    assert n >= 16
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_event_counts(torch.zeros(1, 2, 3, 3))
    with pytest.raises(ValueError, match="fp32"):
        render_event_counts(torch.zeros(1, 2, 3, 3, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="fp32"):
        render_event_counts(torch.zeros(2, 3, 3, device=dev))
    with pytest.raises(ValueError, match="pixels"):
        render_event_counts(torch.zeros(1, 2, 0, 3, device=dev))


def test_render_event_counts_many_chunks_and_a_batch():
    """180 x 241: a plane spans 43 trips of the select workgroup and the colour grid's last part is ragged (43 380 = 10 x 4 096 +
    2 420 pixels); the batch mixes sparse counts, dense values with negatives and halves that round."""
    dev = _gpu()
    from bmc_hip import slots
    from bmc_hip.encodings import render_event_counts
    rng = np.random.default_rng(180241)
    h, w = 180, 241
    assert slots.render_parts(h, w) == 11 and (h * w) % 4096 != 0
    cnt = np.stack([rng.poisson(0.3, (2, h, w)), rng.normal(0.0, 2.0, (2, h, w)), rng.integers(0, 9, (2, h, w)) * 0.5,
                    np.abs(rng.normal(0.0, 1.2, (2, h, w)))]).astype(np.float32)
    for rnd in (False, True):
        before = slots.RENDER_LAUNCHES
        out = render_event_counts(torch.tensor(cnt).to(dev), round=rnd)
        assert slots.RENDER_LAUNCHES == before + 1                             # one call = two launches for the whole batch
        for b in range(len(cnt)):
            assert _np(out[b]).tobytes() == R.render_np(cnt[b], round=rnd).tobytes(), (b, rnd)
        again = render_event_counts(torch.tensor(cnt).to(dev), round=rnd)
        assert torch.equal(out, again)                                         # the same bytes run after run


def test_render_ranks_that_differ_in_the_last_digit_only():
    """16 x 16 planes whose 256 values are 256 neighbouring float32: the keys of the select agree in their top three digits, so
    the four ranks of the two percentiles share one histogram for three passes and part in the last."""
    dev = _gpu()
    from bmc_hip.encodings import render_event_counts
    rng = np.random.default_rng(1616)
    bits = np.stack([0x40000000 + rng.permutation(256), 0x3F800100 + rng.permutation(256)]).astype(np.uint32)
    cnt = bits.view(np.float32).reshape(2, 16, 16)
    srt = np.sort(bits[0])
    assert len({int(v) >> 8 for v in srt}) == 1 and len({int(srt[k]) & 255 for k in (2, 3, 252, 253)}) == 4
    out = render_event_counts(torch.tensor(cnt)[None].to(dev))
    assert _np(out[0]).tobytes() == R.render_np(cnt).tobytes()


@pytest.mark.parametrize("h,w", [(7, 9), (31, 57), (64, 64)])
def test_slot_render_touches_only_its_slots(h, w):
    """Slot 0 active with a destination at an odd address (byte stores), slot 1 active at an aligned one (word stores), slot 2
    inactive with both pointers set, slot 3 active without a source: the last two are untouched, and so is every guard."""
    dev = _gpu()
    from bmc_hip import slots
    rng = np.random.default_rng(h * w)
    S, n = 4, h * w
    cnt = torch.tensor(rng.poisson(0.8, (S, 2, h, w)).astype(np.float32)).to(dev)
    stride = (3 * n + 2 * GUARD + 15) // 16 * 16
    buf = torch.full((S * stride + 16,), 77, dtype=torch.uint8, device=dev)
    base = buf.data_ptr() + (-buf.data_ptr()) % 16
    off = [s * stride + GUARD + (1 if s == 0 else 0) + (base - buf.data_ptr()) for s in range(S)]
    assert (buf.data_ptr() + off[0]) % 4 == 1 and (buf.data_ptr() + off[1]) % 4 == 0
    table = slots.SlotTable(S, dev, render=2)
    e = table.host()
    rn = table.render_host()
    for s in range(S):
        e[s]["frames"], e[s]["flags"] = cnt[s].data_ptr(), 0 if s == 2 else slots.ACTIVE
        rn[1, s]["src"], rn[1, s]["dst"] = 0 if s == 3 else cnt[s].data_ptr(), buf.data_ptr() + off[s]
    table.upload()
    scratch = torch.zeros(4 * S, device=dev)
    slots.render(table, 1, h, w, False, scratch)
    torch.cuda.synchronize()
    keep = torch.ones_like(buf, dtype=torch.bool)
    for s in (0, 1):
        got = buf[off[s]:off[s] + 3 * n]
        assert _np(got).tobytes() == R.render_np(_np(cnt[s])).tobytes(), s
        keep[off[s]:off[s] + 3 * n] = False
    assert (buf[keep] == 77).all()
    slots.render(table, 0, h, w, False, scratch)                               # table 0 has no entries: nothing is written
    torch.cuda.synchronize()
    assert (buf[keep] == 77).all()
    with pytest.raises(ValueError, match="no render tables"):
        slots.render(slots.SlotTable(S, dev), 0, h, w, False, scratch)
    with pytest.raises(ValueError, match="render tables"):
        slots.render(table, 2, h, w, False, scratch)
    with pytest.raises(ValueError, match="pixels"):
        slots.render(table, 0, 4097, 4096, False, scratch)
    with pytest.raises(ValueError, match="scratch"):
        slots.render(table, 0, h, w, False, scratch[:4 * S - 1])


# ------------------------------------------------------------------ (b) sessions
H_, W_ = 12, 20
WINDOWS = (4, 6, 3, 5)


@functools.lru_cache(maxsize=None)
def _case(H, W, gh, gw, seed):
    return _recordings(WINDOWS, H, W, gh, gw, seed)


@functools.lru_cache(maxsize=None)
def _session(graph, S=3, only=None):
    """The rendering session on the four recordings (or on recording `only` alone) -> (results per recording, recordings)."""
    dev = _gpu()
    from infer import MultiStreamSR
    m = _model(False, N_C, seed=307).to(dev)
    recs = [(f.to(dev), g.to(dev)) for f, g in _case(H_, W_, SCALE * H_, SCALE * W_, 31)]
    if only is not None:
        recs = [recs[only]]
    ms = MultiStreamSR(m, S, n_c=N_C, scale=SCALE, graph=graph, keep_predictions=True, render=ALL)
    hs = [ms.open(f, g) for f, g in recs]
    empty = False
    while ms.step():
        empty |= any(s is None for s in ms.sched.slots)                        # (the slots as the window just run had them)
    if graph:
        assert ms._graph is not None and ms.replays > 0
    if only is None:
        assert empty and len(recs) > S                                         # a slot was reused, and one stood empty
    torch.cuda.synchronize()
    return [ms.results(h) for h in hs], recs


def _check_images(res, frames, gts, gt_size, what):
    """Every image of a recording's results against the restatement of the tensors the session exposes."""
    from bmc_hip import ops
    imgs = res["images"]
    pred = res["predictions"]
    n = len(pred)
    assert n == len(frames) - SEQN + 1 and all(len(t) == n for t in imgs.values())
    for i in range(n):
        _same(imgs["lr"][i], frames[i + 1], what=(what, "lr", i))
        if gts is None:
            _same(imgs["esr"][i], pred[i], round=True, what=(what, "esr", i))
            continue
        esr = ops.bicubic_resize(pred[i:i + 1], gt_size)[0]                    # (the identity when the sizes agree)
        _same(imgs["esr"][i], esr, round=True, what=(what, "esr", i))
        _same(imgs["bicubic"][i], ops.bicubic_resize(frames[i + 1:i + 2].contiguous(), gt_size)[0], what=(what, "bicubic", i))
        _same(imgs["gt"][i], gts[i + 1], what=(what, "gt", i))


@pytest.mark.parametrize("graph", [False, True])
def test_session_images_equal_the_restatement(graph):
    res, recs = _session(graph)
    for k, (r, (f, g)) in enumerate(zip(res, recs)):
        assert set(r["images"]) == set(ALL)
        assert tuple(r["images"]["lr"].shape[1:]) == (H_, W_, 3) and tuple(r["images"]["esr"].shape[1:]) == (SCALE * H_, SCALE * W_, 3)
        _check_images(r, f, g, (SCALE * H_, SCALE * W_), (graph, k))
    assert any((_np(r["images"]["esr"]) != 255).any() for r in res)            # pictures, not blank sheets


def test_eager_and_graph_sessions_are_byte_identical():
    eager, graph = _session(False)[0], _session(True)[0]
    for a, b in zip(eager, graph):
        assert torch.equal(a["predictions"], b["predictions"])
        for k in ALL:
            assert torch.equal(a["images"][k], b["images"][k]), k


def test_a_recording_alone_gives_the_same_images():
    beside = _session(False)[0][1]
    alone = _session(False, S=1, only=1)[0][0]
    assert torch.equal(alone["predictions"], beside["predictions"])
    for k in ALL:
        assert torch.equal(alone["images"][k], beside["images"][k]), k


@pytest.mark.parametrize("graph", [False, True])
def test_recordings_without_ground_truth_and_a_resized_prediction(graph):
    """12 x 22 sensor, 46 x 86 ground truth: the prediction (48 x 88) is resized for the esr image of a recording with ground
    truth; a recording without one gets lr and esr at 48 x 88 only.  The session starts without ground truth: its first
    recording with one joins after the capture and invalidates the graph."""
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    H, W, gh, gw = 12, 22, 46, 86
    m = _model(False, N_C, seed=311).to(dev)
    recs = [(f.to(dev), g.to(dev)) for f, g in _case(H, W, gh, gw, 37)]
    ms = MultiStreamSR(m, 2, n_c=N_C, scale=SCALE, graph=graph, keep_predictions=True, render=ALL)
    hs = [ms.open(recs[0][0]), ms.open(recs[1][0])]
    assert ms.scratch_bytes() == 4 * 4 * 2
    for _ in range(3):
        ms.step()
    assert (ms._graph is not None) == graph and "render_resize" not in ms._bufs
    hs += [ms.open(recs[2][0], recs[2][1]), ms.open(recs[3][0], recs[3][1], gt_size=(gh, gw))]
    assert ms._graph is None and tuple(ms._bufs["render_resize"].shape) == (2, 2, gh, gw)
    assert ms.scratch_bytes() == 4 * 4 * 2 + 4 * 2 * 2 * (gh * gw + H * W)
    ms.run()
    if graph:
        assert ms._graph is not None and ms.replays > 0
    for k, h in enumerate(hs):
        r = ms.results(h)
        f, g = recs[k]
        if k < 2:
            assert set(r["images"]) == {"lr", "esr"} and "esr_mse" not in r
            assert tuple(r["images"]["esr"].shape[1:]) == (SCALE * H, SCALE * W, 3)
            _check_images(r, f, None, None, (graph, k))
        else:
            assert set(r["images"]) == set(ALL) and all(tuple(r["images"][kind].shape[1:]) == (gh, gw, 3) for kind in ALL[1:])
            _check_images(r, f, g, (gh, gw), (graph, k))
        nwin = len(f) - SEQN + 1
        plain = MultiStreamSR(m, 2, n_c=N_C, scale=SCALE, keep_predictions=True)
        hp = plain.open(f, None if k < 2 else g)
        extra = 3 * nwin * (H * W + SCALE * H * SCALE * W) if k < 2 else 3 * nwin * (H * W + 3 * gh * gw)
        assert ms.resident_bytes(h) == plain.resident_bytes(hp) + extra
    assert slots.RENDER_KERNELS == 2


@pytest.mark.parametrize("graph", [False, True])
def test_event_backed_filtered_session_renders_the_filtered_frame(graph):
    dev = _gpu()
    from infer import MultiStreamSR
    from test_gpu_hot_filter import GH, GW, HF, _dev, _gt_frames, _session_recordings
    from test_gpu_hot_filter import H_ as EH, W_ as EW
    m = _model(False, N_C, seed=313).to(dev)
    recs = _session_recordings()[:3]
    ms = MultiStreamSR(m, 2, n_c=N_C, scale=SCALE, graph=graph, keep_predictions=True, hot_filter=HF, render=ALL)
    hs = [ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (EH, EW), (GH, GW)) for lr, li, gt, gi, _ in recs]
    ms.run()
    if graph:
        assert ms.replays > 0
    for k, (h, (_, _, gt, gi, f)) in enumerate(zip(hs, recs)):
        assert not np.array_equal(f["frames"], f["raw"])                       # the filter acted on what lr shows
        _check_images(ms.results(h), torch.tensor(f["frames"]).to(dev), _gt_frames(gt, gi, dev), (GH, GW), (graph, k))


# ------------------------------------------------------------------ (c) the default
def test_without_render_nothing_changes():
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR, evaluate_recordings
    m = _model(False, N_C, seed=317).to(dev)
    recs = [(f.to(dev), g.to(dev)) for f, g in _case(H_, W_, SCALE * H_, SCALE * W_, 31)][:2]

    def session(**kw):
        ms = MultiStreamSR(m, 2, n_c=N_C, scale=SCALE, keep_predictions=True, **kw)
        hs = [ms.open(f, g) for f, g in recs]
        per = []
        while True:
            before = (dict(slots.LAUNCHES), slots.ENCODE_LAUNCHES, slots.EMIT_LAUNCHES, slots.HOT_LAUNCHES, slots.RENDER_LAUNCHES)
            if not ms.step():
                break
            per.append(({k: slots.LAUNCHES[k] - before[0][k] for k in before[0]}, slots.ENCODE_LAUNCHES - before[1],
                        slots.EMIT_LAUNCHES - before[2], slots.HOT_LAUNCHES - before[3], slots.RENDER_LAUNCHES - before[4]))
        return ms, hs, per

    one = {"stage": 1, "commit": 1, "metrics": 1}
    without, h0, per0 = session()
    off, h1, per1 = session(render=None)
    on, h2, per2 = session(render=ALL)
    assert per0 == per1 and all(p == (one, 0, 0, 0, 0) for p in per0)          # the launches of a session without the argument
    assert all(p == (one, 0, 0, 0, 4) for p in per2)                           # on: one call (two launches) per kind, same sizes
    for ms in (without, off):
        t = ms._bufs["table"]
        assert t.render == 0 and t.dev.numel() == slots.table_layout(2)[1] and not any(k.startswith("render") for k in ms._bufs)
        assert ms.scratch_bytes() == 0
    for a, b, c in zip(h0, h1, h2):
        ra, rb, rc = without.results(a), off.results(b), on.results(c)
        for r in (ra, rb, rc):
            r.pop("time")
        assert set(ra) == set(rb) == {"esr_mse", "bicubic_mse", "predictions"} and set(rc) == set(ra) | {"images"}
        assert ra["esr_mse"] == rb["esr_mse"] == rc["esr_mse"] and ra["bicubic_mse"] == rb["bicubic_mse"] == rc["bicubic_mse"]
        assert torch.equal(ra["predictions"], rb["predictions"]) and torch.equal(ra["predictions"], rc["predictions"])
        assert without.resident_bytes(a) == off.resident_bytes(b)
    out = evaluate_recordings(m, recs, 2, n_c=N_C, scale=SCALE, keep_predictions=True)
    assert "images" not in out
    out = evaluate_recordings(m, recs, 2, n_c=N_C, scale=SCALE, render=("esr", "lr"))
    assert set(out["images"]) == {"0", "1"} and set(out["images"]["0"]) == {"lr", "esr"}
    assert torch.equal(out["images"]["1"]["esr"], on.results(h2[1])["images"]["esr"])
    with pytest.raises(ValueError, match="unknown kind"):
        evaluate_recordings(m, recs, 2, n_c=N_C, scale=SCALE, render=("png",))
