"""The two SSIM tile launches share one body (csrc/ssim_k.h): for the same image pair and a constant data range, the float64
tile partials bmc_ssim_loss_fwd writes (tiles[b * 2 + c][tile]) and the ones bmc_slot_quality writes for the esr image
(tiles[s][channel][tile], bicubic None) are the same bits.  Slot 1 holds x == y bit for bit: there A1 == B1 and A2 == B2, S is
exactly 1.0 at every position, and a tile's partial is its count of positions inside the image -- exact in both launches.

Shapes (TH x TW the tile in window positions, 32 x 64 in both headers): one position; exactly one tile; four tiles, three of
them one position thick; twelve ragged tiles.  B = S = 2, C = 2; data ranges 1 and 255; contents ssim_loss_ref.make_pair."""
import numpy as np
import pytest
import torch

import ssim_loss_ref as SR
from bmc_hip import ssim_lib
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401

pytestmark = pytest.mark.gpu

TH, TW = ssim_lib.TILE_H, ssim_lib.TILE_W
SHAPES = [(7, 7), (TH + 6, TW + 6), (TH + 7, TW + 7), (2 * TH + 9, 3 * TW + 11)]
RANGES = [1.0, 255.0]


@pytest.mark.parametrize("R", RANGES)
@pytest.mark.parametrize("shape", SHAPES, ids=["one_position", "one_tile", "four_tiles", "ragged"])
def test_loss_and_quality_tile_partials_are_the_same_bits(shape, R):
    dev = _gpu()
    from bmc_hip import lib, ops, slots
    if (slots.QUALITY_TILE_H, slots.QUALITY_TILE_W) != (TH, TW):
        pytest.skip("bmc_hip_quality.h tiles %d x %d positions and bmc_hip_ssim.h %d x %d: the partials cover other positions, "
                    "nothing to compare" % (slots.QUALITY_TILE_H, slots.QUALITY_TILE_W, TH, TW))
    h, w = shape
    x, y = SR.make_pair(2, 2, h, w, seed=1000 * h + 10 * w + int(R))
    x[1] = y[1]
    x, y = torch.tensor(x).to(dev), torch.tensor(y).to(dev)
    nt = ssim_lib.fwd_tiles(h, w)
    assert nt == slots.quality_tiles(h, w) == [1, 1, 4, 12][SHAPES.index(shape)]

    of_loss = torch.zeros(4 * nt, dtype=torch.float64, device=dev)           # two fills that differ: an unwritten partial shows
    loss = torch.empty((), dtype=torch.float32, device=dev)
    lib.call(ssim_lib._ssim_loss_fwd, "bmc_ssim_loss_fwd", x.data_ptr(), y.data_ptr(), y.stride(0), 2, 2, h, w, R,
             of_loss.data_ptr(), loss.data_ptr(), ops._stream())

    of_quality = torch.full((2 * 4 * nt,), -1.0, dtype=torch.float64, device=dev)
    rec = torch.zeros(2, 2, slots.QUALITY_WORDS, dtype=torch.float64, device=dev)
    nparts = slots.metric_parts(h, w)
    stats = torch.zeros(2 * nparts * slots.QUALITY_STATS_WORDS, dtype=torch.float64, device=dev)
    table = slots.SlotTable(2, dev, quality=True)
    e, qe = table.host(), table.quality_host()
    for s in range(2):
        e[s]["frames"], e[s]["gt"], e[s]["flags"] = y[s].data_ptr(), y[s].data_ptr(), slots.ACTIVE
        qe[s]["dst"] = rec[s].data_ptr()
    table.upload()
    slots.quality(table, x, None, nparts, R, stats, of_quality)
    torch.cuda.synchronize()

    a = of_loss.view(2, 2, nt).cpu()
    b = of_quality.view(2, 4, nt)[:, :2].cpu()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (a - b).abs().max()
    ph, pw = h - 6, w - 6
    inside = [min(TH, ph - ty * TH) * min(TW, pw - tx * TW) for ty in range(-(-ph // TH)) for tx in range(-(-pw // TW))]
    assert np.array_equal(a[1].numpy(), np.broadcast_to(np.asarray(inside, np.float64), (2, nt)))
    assert bool((a[0] != a[1]).any()) and bool(torch.isfinite(a).all())
