"""The event-count renderer's contract on the CPU (include/bmc_hip.h, "event-count images"): the numpy restatement
(tests/event_render_ref.py) against the arrays the reference's plot_event_cnt returned (tests/golden/event_render.npz) and
against an np.percentile-based rendering, and the validation of MultiStreamSR(render=...) and of the tool's --render."""
import os
import sys

import numpy as np
import pytest

import event_render_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def golden_cases():
    """(name, cnt float32 [2,h,w], round, img uint8 [h,w,3]) of every golden."""
    z = np.load(os.path.join(HERE, "golden", "event_render.npz"), allow_pickle=False)
    for k in range(int(z["n"])):
        yield str(z["name_%d" % k]), z["cnt_%d" % k], bool(z["round_%d" % k]), z["img_%d" % k]


def test_the_goldens_cover_the_cases():
    cases = list(golden_cases())
    sizes = {c[1].shape[1:] for c in cases}
    assert {(7, 9), (24, 40), (31, 57), (1, 101), (1, 1), (3, 5)} <= sizes and len(cases) >= 16
    assert all(c[1].dtype == np.float32 and c[1][0].size <= 64 * 64 and c[3].dtype == np.uint8 for c in cases)
    by = {c[0]: c for c in cases}
    assert (by["gaussian_dense"][1] < 0).any() and by["halves_rounded"][2] and (by["halves_rounded"][1] % 1 == 0.5).any()
    assert (by["positive_all_zero"][1][0] == 0).all() and (by["negative_all_zero"][1][1] == 0).all()
    assert len(np.unique(by["constant"][1])) == 1 and by["large_counts_clip"][1].max() > 1e5
    assert os.path.getsize(os.path.join(HERE, "golden", "event_render.npz")) < 200 * 1024


def test_restatement_equals_every_golden():
    for name, cnt, rnd, img in golden_cases():
        got = R.render_np(cnt, round=rnd)
        assert got.dtype == np.uint8 and got.shape == img.shape
        assert got.tobytes() == img.tobytes(), name


def test_constant_image_keeps_the_unnormalised_quirk():
    by = {c[0]: c for c in golden_cases()}
    assert (by["constant"][3] == np.array([0, 0, 255], np.uint8)).all()       # 3.0 stays 3.0, is clipped to 1: full blue
    assert (by["constant_half"][3] == np.array([191, 191, 255], np.uint8)).all()          # 0.25 stays: 1 - 0.25 = 0.75 -> 191
    assert (by["all_zero"][3] == 255).all()


def test_percentile_ranks():
    assert R.percentile_ranks(1) == ((0, 0, 0.0), (0, 0, 0.0))
    (k0, k1, g0), (k2, k3, g1) = R.percentile_ranks(101)                      # both virtual indices integral
    assert (k0, k1, float(g0), k2, k3, float(g1)) == (1, 2, 0.0, 99, 100, 0.0)
    # the virtual index is a float32 product: at 180 x 320 it differs from the float64 one in the gamma
    (_, _, g0), (k2, k3, g1) = R.percentile_ranks(180 * 320)
    assert (k2, k3) == (57023, 57024) and float(g1) == float(np.float32(57599) * (np.float32(99) / np.float32(100))) - 57023
    assert float(g1) != 57599 * 0.99 - 57023


def test_restatement_equals_np_percentile_rendering():
    """A NumPy that changes how it places or interpolates a percentile of a float32 array is noticed here."""
    rng = np.random.default_rng(5)
    for t in range(200):
        h, w = int(rng.integers(1, 70)), int(rng.integers(1, 90))
        if t % 20 == 0:
            h, w = int(rng.integers(150, 200)), int(rng.integers(200, 330))
        kind = t % 4
        if kind == 0:
            cnt = rng.poisson(rng.uniform(0.05, 3.0), (2, h, w))
        elif kind == 1:
            cnt = rng.normal(0.0, 2.0, (2, h, w))
        elif kind == 2:
            cnt = np.abs(rng.normal(0.0, 1.5, (2, h, w)))
        else:
            cnt = rng.integers(0, 7, (2, h, w)) * 0.5
        cnt = cnt.astype(np.float32)
        rnd = bool((t // 4) % 2)
        assert R.render_np(cnt, rnd).tobytes() == R.render_percentile_np(cnt, rnd).tobytes(), (t, h, w)


def test_render_option_validation():
    from infer import MultiStreamSR
    assert MultiStreamSR(_Dummy(), 2).render == ()
    assert MultiStreamSR(_Dummy(), 2, render=("gt", "lr")).render == ("lr", "gt")
    assert MultiStreamSR(_Dummy(), 2, render=["esr"]).render == ("esr",)
    assert MultiStreamSR(_Dummy(), 2, render=MultiStreamSR.RENDER_KINDS).render == ("lr", "bicubic", "esr", "gt")
    for bad, what in (("lr", "tuple"), ((), "tuple"), (("lr", "hr"), "unknown kind 'hr'"), (("lr", "lr"), "twice"),
                      (True, "tuple"), (("lr", 3), "unknown kind 3"), ({"lr": 1}, "tuple")):
        with pytest.raises(ValueError, match=what):
            MultiStreamSR(_Dummy(), 2, render=bad)


class _Dummy:
    def eval(self):
        return self


def test_slot_table_render_section():
    from bmc_hip import lib, slots
    assert "bmc_slot_render" in lib.EXPORTS and lib.has_symbol("bmc_slot_render")
    sections, nbytes = slots.table_layout(3, events=True, render=2)
    assert [s[0] for s in sections] == ["slot", "events", "render"] and nbytes == 3 * (40 + 192 + 2 * 16)
    assert slots.table_layout(3) == slots.table_layout(3, render=0) and slots.table_layout(3)[1] == 120
    for bad in (-1, True, 1.0, slots.MAX_RENDER_TABLES + 1):
        with pytest.raises(ValueError, match="render"):
            slots.table_layout(3, render=bad)
    assert slots.render_parts(1, 1) == 1 and slots.render_parts(180, 241) == 11 and slots.render_parts(4096, 4096) == 1024
    assert slots.RENDER_KERNELS == 2


def test_tool_render_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import multistream_infer as T
    finally:
        sys.path.pop(0)
    a = T.parse_args([])
    assert a.render is None and a.render_kinds is None
    a = T.parse_args(["--render", "out"])
    assert a.render == "out" and a.render_kinds == ("lr", "bicubic", "esr", "gt")
    a = T.parse_args(["--render", "out", "--render-kinds", "gt,lr"])
    assert a.render_kinds == ("lr", "gt")
    for bad in (["--render-kinds", "lr"], ["--render", "out", "--render-kinds", "lr,png"], ["--render", "out", "--render-kinds", ""],
                ["--render"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
    assert T.RENDER_DIRS == {"lr": "lr_event_img", "bicubic": "hr_bicubic_event_img", "esr": "hr_esr_event_img",
                             "gt": "hr_gt_event_img"}


def test_tool_writes_the_arrays_themselves(tmp_path):
    import torch
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import multistream_infer as T
    finally:
        sys.path.pop(0)
    imgs = np.random.default_rng(0).integers(0, 256, (2, 5, 7, 3)).astype(np.uint8)
    T.write_images(str(tmp_path), "rec000", {"esr": torch.from_numpy(imgs)})
    for i in range(2):
        back = np.asarray(Image.open(os.path.join(str(tmp_path), "rec000", "event_img", "hr_esr_event_img", "%09d.png" % i)))
        assert back.tobytes() == imgs[i].tobytes()
