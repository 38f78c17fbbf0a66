"""PSNR / SSIM of multi-stream inference on the MI355X (csrc/slot_quality.hip; include/bmc_hip_quality.h): the three launches on
their own through bmc_hip.encodings.image_quality at the tile edges, and whole sessions (MultiStreamSR(quality=...)), against
the float64 oracle of tests/quality_ref.py -- never against the kernel.

Bars (quality_ref.py derives them): gt_max / gt_min exact; sse relative SSE_BAR = 1e-12; a channel's mean SSIM absolute
SSIM_BAR = max(1000 * FLOOR, 1e-13) <= 1e-10; a PSNR is 10 log10 of a quotient with sse in it, so a relative 1e-12 of sse moves
it by 10 / ln 10 * 1e-12 = 4.4e-12 -- PSNR_BAR = 1e-11 absolute covers the two channels' log10 roundings too."""
import numpy as np
import pytest
import torch

import quality_ref as Q
from test_gpu_multistream import SCALE, SEQN, _model, _recordings
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401

pytestmark = pytest.mark.gpu

PSNR_BAR = 1e-11
KEYS = ("esr_psnr", "esr_ssim", "bicubic_psnr", "bicubic_ssim")
H, W, N_C = 12, 20, 16


def _tiles():
    from bmc_hip import quality_lib
    return quality_lib.const("BMC_QUALITY_TILE_H"), quality_lib.const("BMC_QUALITY_TILE_W")


def _bits(values):
    return np.asarray(values, np.float64).view(np.int64).tolist()


def _close(got, want, bar, what):
    """Finite values within `bar`, the others (+-inf, nan) the same."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    print(what, "worst", float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0, "bar", bar)
    assert np.array_equal(np.isfinite(got), fin), what
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    assert (np.abs(got[fin] - want[fin]) <= bar).all(), what


# ------------------------------------------------------------------ 1. the kernels alone
# (h, w) by position in quality_ref.shapes(TH, TW): the ids stay put when the header's tile constants change
@pytest.mark.parametrize("k", range(7), ids=["one_position", "7x8", "8x7", "one_tile", "four_tiles", "ragged", "two_parts"])
def test_kernels_vs_float64_oracle(k):
    dev = _gpu()
    from bmc_hip import slots
    from bmc_hip.encodings import image_quality
    h, w = Q.shapes(*_tiles())[k]
    assert k != 6 or slots.metric_parts(h, w) > 1
    a, g = Q.make_images(h, w, seed=h * 1000 + w)
    ta, tg = torch.tensor(a).to(dev), torch.tensor(g).to(dev)
    n0 = slots.QUALITY_LAUNCHES
    for rng in ("gt", 4.0):
        got = image_quality(ta, tg, rng, raw=True)
        want = np.stack([Q.raw_record(x, y, rng) for x, y in zip(a, g)])            # [3, 2 channels, 4]
        raw = got["raw"]
        assert raw.shape == (3, 2, 4) and np.array_equal(raw[..., 1:3], want[..., 1:3])                       # gt_max, gt_min: exact
        sse, ref = raw[..., 0], want[..., 0]
        print(h, w, rng, "sse worst", float((np.abs(sse - ref) / np.where(ref > 0, ref, 1.0)).max()))
        assert (np.abs(sse - ref) <= Q.SSE_BAR * ref).all() and (sse[1] == 0.0).all()
        npos = (h - 6) * (w - 6)
        _close(raw[..., 3] / npos, want[..., 3] / npos, Q.SSIM_BAR, "%dx%d %s ssim_c" % (h, w, rng))
        psnr, ssim = Q.quality(a, g, rng)
        _close(got["psnr"], psnr, PSNR_BAR, "%dx%d %s psnr" % (h, w, rng))
        _close(got["ssim"], ssim, Q.SSIM_BAR, "%dx%d %s ssim" % (h, w, rng))
        assert got["psnr"][1] == np.inf and got["ssim"][1] == 1.0                   # a == g bit for bit
        if rng == "gt":                                                             # channel 1 of g empty: R_1 = 0
            assert got["psnr"][2] == -np.inf and np.isnan(got["ssim"][2]) and np.isnan(raw[2, 1, 3])
        else:
            assert np.isfinite(got["psnr"][2]) and np.isfinite(got["ssim"][2])
        again = image_quality(ta, tg, rng, raw=True)["raw"]
        assert np.array_equal(again.view(np.int64), raw.view(np.int64))              # bit-reproducible
    assert slots.QUALITY_LAUNCHES - n0 == 4


def test_image_quality_refusals():
    dev = _gpu()
    from bmc_hip.encodings import image_quality
    a = torch.zeros(1, 2, 9, 9, device=dev)
    for bad, exc in (((a[:, :1], a), ValueError), ((a, a[..., :8]), ValueError), ((a.double(), a), ValueError),
                     ((a[..., :6], a[..., :6]), ValueError), ((a.cpu(), a.cpu()), RuntimeError)):
        with pytest.raises(exc, match="image_quality"):
            image_quality(*bad)
    with pytest.raises(ValueError, match="data_range"):
        image_quality(a, a, 0.0)


# ------------------------------------------------------------------ 2. sessions
def _run(m, recs, dev, graph=False, S=2, plain=False, **kw):
    """A session over frame-backed recordings [(frames, gts or None)] -> (session, [results])."""
    from infer import MultiStreamSR
    ms = MultiStreamSR(m, S, n_c=N_C, scale=SCALE, plain=plain, graph=graph, keep_predictions=True, **kw)
    hs = [ms.open(f.to(dev), None if g is None else g.to(dev)) for f, g in recs]
    ms.run()
    return ms, [ms.results(h) for h in hs]


def _want(res, frames, gts, rng="gt"):
    """The oracle's four lists for a recording: from its kept predictions and frame 1 of every window (frames: as the model
    saw them), resized with ops.bicubic_resize where the ground truth's size differs."""
    from bmc_hip import ops
    size = gts.shape[-2:]
    n = res["predictions"].shape[0]
    esr = ops.bicubic_resize(res["predictions"].contiguous(), size).cpu().numpy()
    bic = ops.bicubic_resize(frames[1:1 + n].contiguous(), size).cpu().numpy()
    g = gts[1:1 + n].cpu().numpy()
    (ep, es), (bp, bs) = Q.quality(esr, g, rng), Q.quality(bic, g, rng)
    return dict(esr_psnr=ep, esr_ssim=es, bicubic_psnr=bp, bicubic_ssim=bs)


def _check(res, want, what):
    for k in KEYS:
        assert len(res[k]) == len(want[k]) == res["predictions"].shape[0] > 0
        _close(res[k], want[k], PSNR_BAR if k.endswith("psnr") else Q.SSIM_BAR, "%s %s" % (what, k))


@pytest.mark.parametrize("rng", ["gt", 2.5])
@pytest.mark.parametrize("gh,gw", [(48, 80), (40, 72)], ids=["same_size", "resized"])
def test_frame_backed_session_vs_oracle(gh, gw, rng):
    dev = _gpu()
    m = _model(False, N_C, seed=41).to(dev)
    recs = _recordings([3, 4, 2], H, W, gh, gw, seed=42)
    ms, res = _run(m, recs, dev, quality=True if rng == "gt" else dict(data_range=rng))
    for (f, g), r in zip(recs, res):
        _check(r, _want(r, f.to(dev), g.to(dev), rng), "frames %dx%d" % (gh, gw))
    finite = [v for r in res for k in KEYS for v in r[k] if np.isfinite(v)]
    assert len(finite) >= 30                                                        # the comparison is not of nans


@pytest.mark.parametrize("gh,gw", [(48, 80), (40, 72)], ids=["same_size", "resized"])
def test_event_backed_session_vs_oracle(gh, gw):
    dev = _gpu()
    from infer import MultiStreamSR
    from test_gpu_event_slots import _dev, _encode_frames, _recording
    m = _model(False, N_C, seed=43).to(dev)
    ms = MultiStreamSR(m, 2, n_c=N_C, scale=SCALE, keep_predictions=True, quality=True)
    recs = [_recording(50 + k, n, H, W, gh, gw) for k, n in enumerate([3, 2, 4])]
    hs = [ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H, W), (gh, gw)) for lr, gt, li, gi in recs]
    ms.run()
    for (lr, gt, li, gi), h in zip(recs, hs):
        r = ms.results(h)
        _check(r, _want(r, _encode_frames(lr, li, H, W, dev), _encode_frames(gt, gi, gh, gw, dev)), "events %dx%d" % (gh, gw))


def test_eager_and_graph_sessions_and_two_runs_give_identical_bits():
    dev = _gpu()
    m = _model(False, N_C, seed=44).to(dev)
    recs = _recordings([6, 5, 3], H, W, 40, 72, seed=45)
    runs = [_run(m, recs, dev, graph=graph, quality=True) for graph in (False, True, True)]
    assert runs[0][0].replays == 0 and runs[1][0].replays > 0
    for ms, res in runs[1:]:
        for r, r0 in zip(res, runs[0][1]):
            for k in KEYS:
                assert _bits(r[k]) == _bits(r0[k]) and len(r[k]) > 0, k


def test_slot_0_does_not_depend_on_slot_1():
    """Recording A in slot 0 while slot 1 is empty, busy with one recording throughout, or taken over mid-session."""
    dev = _gpu()
    m = _model(False, N_C, seed=46).to(dev)
    A, B, C, D = _recordings([5, 5, 2, 2], H, W, 40, 72, seed=47)
    alone = _run(m, [A], dev, quality=True)[1][0]
    for others in ([B], [C, D]):
        ms, res = _run(m, [A] + others, dev, quality=True)
        for k in KEYS:
            assert _bits(res[0][k]) == _bits(alone[k]) and len(alone[k]) == 5, k
        assert all(len(r["esr_ssim"]) == r["predictions"].shape[0] for r in res)


@pytest.mark.parametrize("graph", [False, True])
def test_recording_without_ground_truth_shares_the_session(graph):
    """... and the quality launches join a running (captured) session when the first ground truth arrives."""
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    m = _model(False, N_C, seed=48).to(dev)
    (fa, _), (fb, gb) = _recordings([6, 4], H, W, 40, 72, seed=49)
    ms = MultiStreamSR(m, 2, n_c=N_C, scale=SCALE, graph=graph, keep_predictions=True, quality=True)
    ha = ms.open(fa.to(dev))
    n0 = slots.QUALITY_LAUNCHES
    for _ in range(3):
        assert ms.step()
    assert slots.QUALITY_LAUNCHES == n0 and ms.scratch_bytes() == 0                   # nothing to compare with yet
    hb = ms.open(fb.to(dev), gb.to(dev))
    ms.run()
    ra, rb = ms.results(ha), ms.results(hb)
    assert not set(KEYS) & set(ra) and "esr_mse" not in ra and ra["predictions"].shape[0] == 6
    _check(rb, _want(rb, fb.to(dev), gb.to(dev)), "joined")
    only = _run(m, [(fb, gb)], dev, quality=True)[1][0]
    for k in KEYS:
        assert _bits(rb[k]) == _bits(only[k]), k


def test_self_ensemble_values_are_those_of_the_merged_prediction():
    dev = _gpu()
    m = _model(False, N_C, seed=50).to(dev)
    recs = _recordings([3, 2], H, W, 40, 72, seed=51)
    ms, res = _run(m, recs, dev, self_ensemble=2, quality=True)
    plain = _run(m, recs, dev, quality=True)[1]
    for (f, g), r, p in zip(recs, res, plain):
        assert not torch.equal(r["predictions"], p["predictions"])                   # the merge changes the prediction ...
        _check(r, _want(r, f.to(dev), g.to(dev)), "ensemble")                          # ... and the values are the merged one's
        assert _bits(r["bicubic_psnr"]) == _bits(p["bicubic_psnr"]) and _bits(r["bicubic_ssim"]) == _bits(p["bicubic_ssim"])
        assert _bits(r["esr_ssim"]) != _bits(p["esr_ssim"])


def test_hot_filter_bicubic_values_are_those_of_the_filtered_frame():
    dev = _gpu()
    from infer import MultiStreamSR
    from test_gpu_hot_filter import GH, GW, H_, W_, HF, _dev, _gt_frames, _session_recordings
    m = _model(True, N_C, seed=52).to(dev)
    recs = _session_recordings()[:3]
    runs = {}
    for hot in (True, False):
        ms = MultiStreamSR(m, 2, n_c=N_C, scale=SCALE, plain=True, keep_predictions=True, quality=True, hot_filter=HF if hot else None)
        hs = [ms.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H_, W_), (GH, GW)) for lr, li, gt, gi, _ in recs]
        ms.run()
        runs[hot] = [ms.results(h) for h in hs]
    for (lr, li, gt, gi, f), r, raw in zip(recs, runs[True], runs[False]):
        gts = _gt_frames(gt, gi, dev)
        _check(r, _want(r, torch.tensor(f["frames"]).to(dev), gts), "filtered")
        _check(raw, _want(raw, torch.tensor(f["raw"]).to(dev), gts), "unfiltered")
        assert _bits(r["bicubic_ssim"]) != _bits(raw["bicubic_ssim"])


def test_option_off_changes_nothing_and_on_adds_only_its_keys():
    dev = _gpu()
    from bmc_hip import slots
    m = _model(False, N_C, seed=53).to(dev)
    gh, gw = 40, 72
    recs = _recordings([4, 3], H, W, gh, gw, seed=54)
    counters = lambda: (dict(slots.LAUNCHES), slots.ENCODE_LAUNCHES, slots.EMIT_LAUNCHES, slots.EMIT_TIMED_LAUNCHES,
                        slots.HOT_LAUNCHES, slots.RENDER_LAUNCHES, slots.VOXEL_LAUNCHES)
    moved = lambda a, b: ({k: b[0][k] - a[0][k] for k in a[0]},) + tuple(y - x for x, y in zip(a[1:], b[1:]))
    kw = dict(render=("esr", "bicubic"), voxel_bins=2, emit_events=True)
    c0, q0 = counters(), slots.QUALITY_LAUNCHES
    off, roff = _run(m, recs, dev, **kw)
    c1, q1 = counters(), slots.QUALITY_LAUNCHES
    on, ron = _run(m, recs, dev, quality=True, **kw)
    c2, q2 = counters(), slots.QUALITY_LAUNCHES
    windows = 4                                                                      # two slots: 4 and 3 windows side by side
    assert q1 == q0 and q2 - q1 == windows and moved(c0, c1) == moved(c1, c2)
    assert moved(c0, c1)[0] == {"stage": windows, "commit": windows, "metrics": windows}
    assert not off._bufs["table"].quality and on._bufs["table"].quality
    assert off._bufs["table"].dev.numel() + 8 * 2 == on._bufs["table"].dev.numel()
    # scratch: the off session's is what its parts declare (pictures: percentiles, resize, frames; voxel partials) ...
    S, sH, sW = 2, SCALE * H, SCALE * W
    pictures = 4 * 4 * S + 4 * S * 2 * gh * gw + 4 * S * 2 * H * W
    assert off.scratch_bytes() == pictures + 4 * 2 * S * slots.voxel_parts(sH, sW)
    # ... and the option adds its own counted buffers: stats, tile partials, two resize images, frame 1
    own = 8 * S * slots.metric_parts(gh, gw) * slots.QUALITY_STATS_WORDS + 8 * S * 4 * slots.quality_tiles(gh, gw) \
        + 2 * (4 * S * 2 * gh * gw) + 4 * S * 2 * H * W
    assert on.scratch_bytes() - off.scratch_bytes() == own
    assert own == sum(on._bufs[k].numel() * on._bufs[k].element_size() for k in on._bufs if k.startswith("quality_"))
    same = _run(m, _recordings([4, 3], H, W, sH, sW, seed=54), dev, quality=True)[0]
    assert "quality_resize_esr" not in same._bufs and "quality_resize" in same._bufs   # the same size: no second resize image
    for a, b in zip(roff, ron):
        assert set(b) - set(a) == set(KEYS) and set(a) <= set(b)
        for k in a:
            if k == "time":
                continue
            for x, y in zip(*(torch.utils._pytree.tree_leaves(v[k]) for v in (a, b))):
                assert torch.equal(x, y) if torch.is_tensor(x) else x == y, k
        assert on.resident_bytes(0) - off.resident_bytes(0) == 128 * 4               # 128 bytes per window


def test_open_refuses_a_small_ground_truth():
    dev = _gpu()
    from infer import MultiStreamSR
    m = _model(True, N_C, seed=55).to(dev)
    ms = MultiStreamSR(m, 2, n_c=N_C, scale=SCALE, plain=True, quality=True)
    f = torch.zeros(SEQN, 2, H, W, device=dev)
    with pytest.raises(ValueError, match="at least 7 x 7"):
        ms.open(f, torch.zeros(SEQN, 2, 6, 20, device=dev))
    assert ms._size is None                                                         # a refused recording leaves no trace
    ms.open(f, torch.zeros(SEQN, 2, 7, 9, device=dev))                              # any other size is taken
    ms.run()
    r = ms.results(0)
    assert np.isnan(r["esr_ssim"]).all() and len(r["esr_ssim"]) == 1                 # an empty ground truth: R = 0


def test_evaluate_recordings_means_ignore_non_finite_windows():
    dev = _gpu()
    from infer import evaluate_recordings
    m = _model(True, N_C, seed=56).to(dev)
    (fa, ga), (fb, gb) = _recordings([3, 2], H, W, 40, 72, seed=57)
    gb = gb.clone()
    gb[2, 1] = 0.0                                                                  # window 1 of b: an empty channel
    recs = {"a": (fa.to(dev), ga.to(dev)), "b": (fb.to(dev), gb.to(dev)), "c": (fa.to(dev), None)}
    out = evaluate_recordings(m, recs, 2, n_c=N_C, scale=SCALE, plain=True, quality=True)
    base = evaluate_recordings(m, recs, 2, n_c=N_C, scale=SCALE, plain=True)
    assert set(base["results"]) == {"esr_mse", "bicubic_mse", "time", "params"}
    for k in KEYS:
        assert set(out["results"][k]) == {"a", "b"} and np.isfinite(list(out["results"][k].values())).all()
        assert out["results"][k + "_nonfinite"] == {"a": 0, "b": 1} and out["mean"][k + "_nonfinite"] == 1
        assert out["mean"][k] == (out["results"][k]["a"] + out["results"][k]["b"]) / 2
    assert out["results"]["esr_mse"] == base["results"]["esr_mse"]
