"""The voxel encoders of csrc/scatter.hip on the GPU, byte for byte, where rounding and summation order show: every fixture of
tests/golden/voxel_bins.npz (the reference's own outputs at bin counts whose t * (bins - 1) is inexact, with float weights,
on bin centres, outside the sensor; tests/test_voxel_bins_cpu.py proves that these inputs tell a fused multiply-add from the
reference's two roundings), batched frames and long per-pixel segments against the numpy oracle that the same fixtures pin,
and more long segments than voxel_sort_long_kernel queues (1 024), through all three encoders that share it."""
import numpy as np
import pytest
import torch

from oracle import bmc_oracle as O
from test_gpu_r2 import _gpu
from test_voxel_bins_cpu import CASES, T_TAGS, V_TAGS, bits

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _dev(dev, *cols):
    return [torch.tensor(np.ascontiguousarray(a, np.float32), device=dev) for a in cols]


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    n = int((bits(got) != bits(want)).sum())
    print("%s: %d of %d elements differ" % (what, n, want.size))
    assert n == 0, what


# ------------------------------------------------------------------ the reference's bytes, every fixture
@pytest.mark.parametrize("tag", V_TAGS)
def test_events_to_voxel_returns_the_reference_bytes(tag):
    dev = _gpu()
    from bmc_hip import encodings as E
    c = CASES[tag]
    runs = []
    for _ in range(2):
        xs, ys, ts, ps = _dev(dev, c["xs"], c["ys"], c["ts"], c["ps"])
        vox = E.events_to_voxel(xs, ys, ts, ps, c["bins"], sensor_size=(c["H"], c["W"]))
        runs.append((_np(vox), _np(xs), _np(ys)))
        assert np.array_equal(bits(_np(ts)), bits(c["ts"])) and np.array_equal(bits(_np(ps)), bits(c["ps"]))
    _same(runs[0][0], c["vox"], tag + " grid")
    _same(runs[0][1], c["xs_after"], tag + " xs")
    _same(runs[0][2], c["ys_after"], tag + " ys")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs)), "a second run gives other bytes"


@pytest.mark.parametrize("tag", T_TAGS)
def test_events_to_voxel_torch_returns_the_reference_bytes(tag):
    dev = _gpu()
    from bmc_hip import encodings as E
    c = CASES[tag]
    runs = []
    for _ in range(2):
        xs, ys, ts, ps = _dev(dev, c["xs"], c["ys"], c["ts"], c["ps"])
        vox = E.events_to_voxel_torch(xs, ys, ts, ps, c["bins"], sensor_size=(c["H"], c["W"]))
        runs.append((_np(vox), _np(xs), _np(ys)))
        assert np.array_equal(bits(_np(ts)), bits(c["ts"])) and np.array_equal(bits(_np(ps)), bits(c["ps"]))
    _same(runs[0][0], c["vox"], tag + " grid")
    _same(runs[0][1], c["xs_after"], tag + " xs")
    _same(runs[0][2], c["ys_after"], tag + " ys")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs)), "a second run gives other bytes"


# ------------------------------------------------------------------ batched frames against the oracle
@pytest.mark.parametrize("bins,H,W", [(7, 9, 11), (10, 6, 9)])
def test_batched_frames_float_weights(bins, H, W):
    """Three frames, the middle one empty, float weights, events up to a pixel outside the sensor; mutate=False returns the
    same grids and leaves the coordinates alone."""
    dev = _gpu()
    from bmc_hip import ops
    rng = np.random.default_rng(100 * bins + W)
    counts = [300, 0, 350]
    n = sum(counts)
    bounds = np.concatenate([[0], np.cumsum(counts)])
    xs = (rng.integers(-4, 4 * W + 5, n) / 4.0).astype(np.float32)
    ys = (rng.integers(-4, 4 * H + 5, n) / 4.0).astype(np.float32)
    ts = np.concatenate([np.sort(rng.uniform(0, 1, k)) for k in counts]).astype(np.float32)
    ps = rng.standard_normal(n).astype(np.float32)
    off = torch.tensor(bounds, dtype=torch.int64, device=dev)
    d = _dev(dev, xs, ys, ts, ps)
    keep = ops.events_to_voxel_batched(d[0], d[1], d[2], d[3], off, bins, H, W, mutate=False)
    assert np.array_equal(bits(_np(d[0])), bits(xs)) and np.array_equal(bits(_np(d[1])), bits(ys)), "mutate=False wrote coordinates"
    got = ops.events_to_voxel_batched(d[0], d[1], d[2], d[3], off, bins, H, W, mutate=True)
    assert tuple(got.shape) == (3, bins, H, W)
    assert _np(keep).tobytes() == _np(got).tobytes(), "mutate=False gives another grid than mutate=True"
    for f in range(3):
        a, b = bounds[f], bounds[f + 1]
        ref, xa, ya = O.events_to_voxel_np(xs[a:b], ys[a:b], ts[a:b], ps[a:b], bins, (H, W))
        _same(_np(got[f]), ref, "frame %d grid" % f)
        _same(_np(d[0][a:b]), xa, "frame %d xs" % f)
        _same(_np(d[1][a:b]), ya, "frame %d ys" % f)
    assert not _np(got[1]).any()


# ------------------------------------------------------------------ long segments: the order decides the bytes
def test_long_segments_float_weights():
    """One hot pixel with 200 events and 150 events outside the sensor (one segment, at [H-1, 0]) among scattered ones: both are
    longer than VOX_LONG and are put in event order by the whole workgroup; with float weights any other order gives other bytes."""
    dev = _gpu()
    from bmc_hip import encodings as E, ops
    H, W, bins, n = 9, 11, 6, 600
    rng = np.random.default_rng(61)
    xs = (rng.integers(0, 4 * W, n) / 4.0).astype(np.float32)
    ys = (rng.integers(0, 4 * H, n) / 4.0).astype(np.float32)
    sel = rng.permutation(n)
    xs[sel[:200]], ys[sel[:200]] = 4.5, 3.25
    xs[sel[200:350]] = rng.choice([-0.25, W, W + 2.0], 150).astype(np.float32)
    ts = np.sort(rng.uniform(0, 1, n)).astype(np.float32)
    ps = rng.standard_normal(n).astype(np.float32)
    ref, xa, ya = O.events_to_voxel_np(xs, ys, ts, ps, bins, (H, W))
    assert np.count_nonzero((xa == 0) & (ya == 0)) >= 150
    d = _dev(dev, xs, ys, ts, ps)
    got = ops.events_to_voxel_batched(d[0], d[1], d[2], d[3], torch.tensor([0, n], dtype=torch.int64, device=dev), bins, H, W)
    _same(_np(got[0]), ref, "grid")
    _same(_np(d[0]), xa, "xs")
    _same(_np(d[1]), ya, "ys")
    # the same segments through the cell machinery of the torch-tensor encoder (integer-valued positions, raw timestamps)
    xi, yi, tr = np.floor(xs), np.floor(ys), (1.5 + 0.03 * ts.astype(np.float64)).astype(np.float32)
    a, b = xi.copy(), yi.copy()
    ref = O.events_to_voxel_torch_np(a, b, tr, ps.copy(), bins, (H, W))
    d = _dev(dev, xi, yi, tr, ps)
    got = E.events_to_voxel_torch(d[0], d[1], d[2], d[3], bins, sensor_size=(H, W))
    _same(_np(got), ref, "torch grid")
    _same(_np(d[0]), a, "torch xs")
    _same(_np(d[1]), b, "torch ys")


# ------------------------------------------------------------------ more long segments than the cooperative sort queues
QUEUE = 1024            # voxel_sort_long_kernel's queue; the segments beyond it are sorted by their pixel's own thread
LONG = 32               # VOX_LONG


@pytest.fixture(scope="module")
def crowd():
    """33 .. 47 events on every one of 40 x 30 = 1 200 pixels, shuffled, plus 40 outside the sensor: every segment is long."""
    H, W = 40, 30
    rng = np.random.default_rng(4030)
    per = rng.integers(LONG + 1, LONG + 16, H * W)
    pix = np.concatenate([np.repeat(np.arange(H * W), per), np.full(40, -1)])
    pix = pix[rng.permutation(len(pix))]
    n = len(pix)
    xs = np.where(pix < 0, W + 0.5, pix % W + rng.integers(0, 4, n) / 4.0).astype(np.float32)
    ys = np.where(pix < 0, 2.0, pix // W + rng.integers(0, 4, n) / 4.0).astype(np.float32)
    ts = np.sort(rng.uniform(0, 1, n)).astype(np.float32)
    ps = rng.standard_normal(n).astype(np.float32)
    assert 45000 < n < 51000 and per.min() > LONG and H * W > QUEUE
    return H, W, xs, ys, ts, ps


def test_queue_overflow_voxel(crowd):
    dev = _gpu()
    from bmc_hip import ops
    H, W, xs, ys, ts, ps = crowd
    bins, n = 4, len(xs)
    ref, xa, ya = O.events_to_voxel_np(xs, ys, ts, ps, bins, (H, W))
    d = _dev(dev, xs, ys, ts, ps)
    got = ops.events_to_voxel_batched(d[0], d[1], d[2], d[3], torch.tensor([0, n], dtype=torch.int64, device=dev), bins, H, W)
    _same(_np(got[0]), ref, "grid")
    _same(_np(d[0]), xa, "xs")
    _same(_np(d[1]), ya, "ys")


def test_queue_overflow_voxel_torch(crowd):
    dev = _gpu()
    from bmc_hip import encodings as E
    H, W, xs, ys, ts, ps = crowd
    xi, yi, tr = np.floor(xs), np.floor(ys), (1.5 + 0.03 * ts.astype(np.float64)).astype(np.float32)
    a, b = xi.copy(), yi.copy()
    ref = O.events_to_voxel_torch_np(a, b, tr, ps.copy(), 4, (H, W))
    d = _dev(dev, xi, yi, tr, ps)
    got = E.events_to_voxel_torch(d[0], d[1], d[2], d[3], 4, sensor_size=(H, W))
    _same(_np(got), ref, "grid")
    _same(_np(d[0]), a, "xs")
    _same(_np(d[1]), b, "ys")


def test_queue_overflow_bilinear_image(crowd):
    dev = _gpu()
    from bmc_hip import encodings as E
    H, W, xs, ys, ts, ps = crowd
    a, b, c = xs.copy(), ys.copy(), ps.copy()
    ref = O.events_to_image_torch_np(a, b, c, (H, W), interpolation="bilinear")
    d = _dev(dev, xs, ys, ps)
    got = E.events_to_image_torch(d[0], d[1], d[2], sensor_size=(H, W), interpolation="bilinear")
    _same(_np(got), ref, "image")
    _same(_np(d[0]), a, "xs")
    _same(_np(d[1]), b, "ys")
    _same(_np(d[2]), c, "ps")
