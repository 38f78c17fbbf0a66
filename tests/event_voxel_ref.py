"""The numpy restatement of the per-window voxel grid (include/bmc_hip.h, "voxel grids"), shared by test_event_voxel_cpu.py
and test_gpu_event_voxel.py: what bmc_slot_voxel must produce byte for byte -- per output pixel, from its two counts."""
import numpy as np

from event_output_ref import quantise_np
from event_times_ref import T0, T1, emit_timed_np, times_np

F = np.float32


def voxel_np(P, bins, max_count=255):
    """P [2,sH,sW] -> float32 [bins,sH,sW]: the contract's rules 1-5 in float32, every operation rounded on its own."""
    assert 1 <= max_count <= 255 and 1 <= bins <= 32
    q = quantise_np(P, max_count)
    _, sH, sW = q.shape
    out = np.zeros((bins, sH, sW), F)
    if int(q.sum()) <= 3:                                  # rule 1
        return out
    t_first = F(T0)                                        # rule 2
    t_last = F(T1) if int(q.max()) >= 2 else F(T0)
    dt = F(F(t_last - t_first) + F(1e-6))
    bm1 = F(bins - 1)
    b = np.arange(bins, dtype=F)
    for row, x in zip(*np.nonzero(q.sum(0))):
        q0, q1 = int(q[0, row, x]), int(q[1, row, x])
        d0, d1 = max(q0 - 1, 1), max(q1 - 1, 1)
        i0 = i1 = 0
        acc = np.zeros(bins, F)
        while i0 < q0 or i1 < q1:                          # rule 4: the exact rational, channel 0 first on ties
            take0 = i1 >= q1 or (i0 < q0 and i0 * d1 <= i1 * d0)
            if take0:
                t, p, i0 = times_np(i0, q0), F(1), i0 + 1  # rule 3
            else:
                t, p, i1 = times_np(i1, q1), F(-1), i1 + 1
            tn = F(F(F(t - t_first) / dt) * bm1)           # rule 5
            w = np.maximum(F(0), F(1) - np.abs(tn - b)).astype(F)
            acc = (acc + p * w).astype(F)
        out[:, sH - 1 - row, x] = acc                      # the grid's rows are the sensor's y
    return out


def stream_columns_np(P, max_count=255):
    """P [2,sH,sW] -> the float32 columns (xs, ys, ts, ps) of the timed stream, as events_to_voxel_torch takes them."""
    xs, ys, ps, ts, _ = emit_timed_np(P, max_count)
    return xs.astype(F), ys.astype(F), ts.astype(F), ps.astype(F)


def voxel_torch_restated(xs, ys, ts, ps, bins, sH, sW):
    """events_to_voxel_torch (dataloader/encodings.py:100-148, temporal_bilinear=True) restated on the installed torch (CPU),
    line by line: the composition the per-pixel form must equal."""
    import torch
    xs, ys, ts, ps = (torch.from_numpy(np.ascontiguousarray(v)) for v in (xs, ys, ts, ps))
    if len(ts) <= 3 or ts.sum() == 0:
        return np.zeros((bins, sH, sW), F)
    dt = ts[-1] - ts[0] + 1e-6
    t_norm = (ts - ts[0]) / dt * (bins - 1)
    zeros = torch.zeros(t_norm.size())
    grids = []
    for bi in range(bins):
        weights = ps * torch.max(zeros, 1.0 - torch.abs(t_norm - bi))
        img = torch.zeros(sH, sW)
        img.index_put_((ys.long(), xs.long()), weights, accumulate=True)
        grids.append(img)
    return torch.stack(grids).numpy()
