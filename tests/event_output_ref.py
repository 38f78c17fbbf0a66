"""The numpy restatement of the emitted event stream (include/bmc_hip.h, bmc_slot_emit), shared by test_event_output_cpu.py
and test_gpu_event_output.py: what the GPU kernels must produce byte for byte."""
import numpy as np


def quantise_np(P, max_count=255):
    """q = min(rint(v), max_count) for v > 0, else 0 (NaN -> 0, +inf -> max_count); rint is round-half-to-even."""
    P = np.asarray(P, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(P > 0, np.minimum(np.rint(P), np.float32(max_count)), 0).astype(np.int64)


def emit_np(P, max_count=255):
    """P [2,sH,sW] -> (xs int16, ys int16, ps int8, q): element (c, row, x), in flat order, gives q identical events
    (x, sH-1-row, +1 for channel 0 / -1 for channel 1)."""
    q = quantise_np(P, max_count)
    c, row, x = np.nonzero(q)                              # C order: channel 0 first, rows top to bottom, x ascending
    k = q[c, row, x]
    return (np.repeat(x, k).astype(np.int16), np.repeat(q.shape[1] - 1 - row, k).astype(np.int16),
            np.repeat(np.where(c == 0, 1, -1), k).astype(np.int8), q)


def counts_np(xs, ys, ps, sH, sW):
    """The count image of an emitted (in-range) stream, as the encoders build it with flags 0: [2,sH,sW] int64."""
    img = np.zeros((2, sH, sW), np.int64)
    np.add.at(img, ((np.asarray(ps) < 0).astype(np.int64), sH - 1 - np.asarray(ys, np.int64), np.asarray(xs, np.int64)), 1)
    return img
