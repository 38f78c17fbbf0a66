"""The per-window voxel grid's contract on the CPU (include/bmc_hip.h, "voxel grids"): the per-pixel numpy restatement
(tests/event_voxel_ref.py) against the grids the reference's events_to_voxel_torch returned (tests/golden/voxel_output.npz)
and against the installed torch's restatement of the composition (timed stream -> events_to_voxel_torch), and the argument
checks of MultiStreamSR(voxel_bins=...), counts_to_voxel and table_layout(voxel=) that need no GPU."""
import os
import sys

import numpy as np
import pytest

import event_voxel_ref as V

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def golden_cases():
    """(name, q int64 [2,sH,sW], bins, vox float32 [bins,sH,sW]) of every golden."""
    z = np.load(os.path.join(HERE, "golden", "voxel_output.npz"), allow_pickle=False)
    for k in range(int(z["n"])):
        yield str(z["name_%d" % k]), z["q_%d" % k], int(z["bins_%d" % k]), z["vox_%d" % k]


def test_the_goldens_cover_the_cases():
    cases = list(golden_cases())
    times = np.load(os.path.join(HERE, "golden", "event_times.npz"), allow_pickle=False)
    for k in range(4):
        for bins in (1, 2, 5, 32):
            name, q, b, vox = cases[4 * k + (1, 2, 5, 32).index(bins)]
            assert name == "event_times_q%d_bins%d" % (k, bins) and b == bins and (q == times["q%d" % k]).all()
            assert vox.dtype == np.float32 and vox.shape == (bins,) + q.shape[1:]
    by = {c[0]: c for c in cases}
    assert by["three_events"][1].sum() == 3 and not by["three_events"][3].any()
    assert by["four_events"][1].sum() == 4 and by["four_events"][3].any()
    assert by["counts_0_or_1"][1].max() == 1 and by["counts_0_or_1"][1].sum() > 3 and by["counts_0_or_1"][3].any()
    assert len(cases) == 19 and os.path.getsize(os.path.join(HERE, "golden", "voxel_output.npz")) < 100 * 1024


def test_restatement_equals_every_golden():
    for name, q, bins, vox in golden_cases():
        got = V.voxel_np(q.astype(np.float32), bins)
        assert got.dtype == np.float32 and got.shape == vox.shape
        assert got.tobytes() == vox.tobytes(), name


def random_image(rng, t):
    """A prediction with fractional, negative, NaN and above-max_count values; the count levels differ from image to image."""
    sH, sW = int(rng.integers(1, 12)), int(rng.integers(1, 14))
    kind = t % 4
    if kind == 0:
        P = rng.poisson(rng.uniform(0.2, 3.0), (2, sH, sW)) + rng.uniform(-0.5, 0.5, (2, sH, sW))
    elif kind == 1:
        P = rng.normal(0.0, 4.0, (2, sH, sW))
    elif kind == 2:
        P = rng.choice([0.0, 0.0, 0.5, 1.0, 1.5, 2.5, 3.0, 17.0, 64.49, 254.5, 255.5, 300.0, -3.0], (2, sH, sW))
    else:
        P = (rng.random((2, sH, sW)) < 0.3) * rng.uniform(0.6, 1.4, (2, sH, sW))           # counts 0 or 1: dt = 1e-6
    P = P.astype(np.float32)
    if t % 3 == 0:
        P.reshape(-1)[int(rng.integers(0, P.size))] = np.nan
    return P


def test_restatement_equals_the_composition():
    """voxel_np (per pixel) == events_to_voxel_torch, restated on the installed torch, of the timed stream's columns."""
    rng = np.random.default_rng(11)
    nonzero = 0
    for t in range(120):
        P = random_image(rng, t)
        max_count = (255, 7, 40)[t % 3]
        bins = (1, 2, 5, 32, 3, 9)[t % 6]
        cols = V.stream_columns_np(P, max_count)
        want = V.voxel_torch_restated(*cols, bins, P.shape[1], P.shape[2])
        got = V.voxel_np(P, bins, max_count)
        assert got.tobytes() == want.astype(np.float32).tobytes(), (t, P.shape, bins, max_count)
        nonzero += bool(got.any())
    assert nonzero > 60


def test_three_events_or_fewer_give_zeros():
    P = np.zeros((2, 4, 5), np.float32)
    P[0, 1, 1], P[1, 3, 4] = 2.2, 1.0                      # N = 3
    assert not V.voxel_np(P, 5).any()
    assert not V.voxel_torch_restated(*V.stream_columns_np(P), 5, 4, 5).any()
    P[0, 0, 0] = 0.7                                       # N = 4
    got = V.voxel_np(P, 5)
    assert got.any() and got.tobytes() == V.voxel_torch_restated(*V.stream_columns_np(P), 5, 4, 5).tobytes()
    assert got[0, 3, 0] == 1.0 and got[4, 2, 1] != 0       # the rows are flipped: P[0,0,0] lands on y = 3; the last event in bin 4
    P[:] = 300.0                                           # clamped by max_count = 1: four events or more, every time 0.01
    got = V.voxel_np(P[:, :1, :2], 3, max_count=1)
    assert not got.any()                                   # +1 and -1 cancel on every pixel
    assert V.voxel_np(np.stack([P[0, :1, :4], 0 * P[0, :1, :4]]), 3, max_count=1)[0].tolist() == [[1.0] * 4]


class _Dummy:
    def eval(self):
        return self


def test_voxel_bins_option_validation():
    from infer import MultiStreamSR
    assert MultiStreamSR(_Dummy(), 2).voxel_bins is None
    assert MultiStreamSR(_Dummy(), 2, voxel_bins=5).voxel_bins == 5
    assert MultiStreamSR(_Dummy(), 2, voxel_bins=np.int64(32), emit_events=True, event_times="linear", render=("esr",)).voxel_bins == 32
    assert MultiStreamSR.MAX_VOXEL_BINS == 32
    for bad in (0, 33, -1, True, 5.0, "5", (5,)):
        with pytest.raises(ValueError, match="voxel_bins"):
            MultiStreamSR(_Dummy(), 2, voxel_bins=bad)
    with pytest.raises(ValueError, match="voxel_bins needs max_count <= 255"):
        MultiStreamSR(_Dummy(), 2, voxel_bins=5, max_count=256)
    assert MultiStreamSR(_Dummy(), 2, max_count=256).voxel_bins is None      # without the option the larger counts stay allowed


def test_counts_to_voxel_argument_errors():
    import torch
    from bmc_hip import encodings
    P = torch.zeros(1, 2, 4, 5)
    for bad, what in ((torch.zeros(2, 4, 5), "fp32 .B,2,sH,sW."), (torch.zeros(1, 3, 4, 5), "fp32 .B,2,sH,sW."),
                      (P.double(), "fp32 .B,2,sH,sW."), (P.numpy(), "fp32 .B,2,sH,sW.")):
        with pytest.raises(ValueError, match=what):
            encodings.counts_to_voxel(bad, 5)
    for bins in (0, 33, True, 2.0):
        with pytest.raises(ValueError, match="bins"):
            encodings.counts_to_voxel(P, bins)
    for mc in (0, 256, True, 3.0):
        with pytest.raises(ValueError, match="max_count"):
            encodings.counts_to_voxel(P, 5, max_count=mc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        encodings.counts_to_voxel(P, 5)


def test_slot_table_voxel_section():
    from bmc_hip import lib, slots
    assert "bmc_slot_voxel" in lib.EXPORTS and lib.has_symbol("bmc_slot_voxel")
    sections, nbytes = slots.table_layout(3, events=True, render=2, voxel=True)
    assert [s[0] for s in sections] == ["slot", "events", "render", "voxel"] and nbytes == 3 * (40 + 192 + 2 * 16 + 8)
    assert sections[-1][1] is slots.SLOT_VOXEL_DTYPE and sections[-1][2] == 3 * (40 + 192 + 2 * 16)
    assert slots.table_layout(3) == slots.table_layout(3, voxel=False) and slots.table_layout(3)[1] == 120
    assert slots.table_layout(3, True, True, True, True, True, 2) == slots.table_layout(3, True, True, True, True, True, 2, False)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="voxel"):
            slots.table_layout(3, voxel=bad)
    assert slots.voxel_parts(1, 1) == 1 and slots.voxel_parts(36, 48) == 1 and slots.voxel_parts(70, 130) == 5
    assert slots.voxel_parts(720, 960) == 338 and slots.voxel_parts(32767, 32767) == 1024
    assert slots.VOXEL_KERNELS == 2 and slots.MAX_VOXEL_BINS == 32 and slots.VOXEL_LAUNCHES == 0


def test_slot_voxel_struct_layout_matches_header():
    import abi_ref
    from bmc_hip import slots
    structs, constants = abi_ref.compiled_header()
    size, compiled = structs["bmc_slot_voxel_t"]
    dt = slots.SLOT_VOXEL_DTYPE
    assert [size, compiled["dst"][0], compiled["dst"][1], constants["BMC_SLOT_VOXEL_MAX_BINS"], constants["BMC_SLOT_EMIT_TIMED_MAX_COUNT"],
            structs["bmc_slot_render_t"][0]] == [dt.itemsize, dt.fields["dst"][1], 8, slots.MAX_VOXEL_BINS, slots.MAX_COUNT_TIMED,
                                                 slots.SLOT_RENDER_DTYPE.itemsize]
    assert dt.names == ("dst",) and dt.itemsize == 8


def test_tool_voxel_argument():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import multistream_infer as T
    finally:
        sys.path.pop(0)
    assert T.parse_args([]).voxel_bins is None
    assert T.parse_args(["--voxel-bins", "5"]).voxel_bins == 5
    for bad in (["--voxel-bins", "0"], ["--voxel-bins", "33"], ["--voxel-bins", "x"], ["--voxel-bins"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
