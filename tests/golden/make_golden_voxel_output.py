#!/usr/bin/env python3
"""Golden voxel grids for the per-window voxel output (include/bmc_hip.h, "voxel grids"): what the REFERENCE's own
events_to_voxel_torch (dataloader/encodings.py:100-148, temporal_bilinear=True) returns for the timed event stream of small
quantised count images (build container only: the reference is imported from BMC_REFERENCE; it ran unpatched under the
installed torch).  The stream is emit_timed_np(q)'s columns as float32 (tests/event_times_ref.py; test_event_times_cpu.py ties
those columns to the reference's own cloud).  Only data is written: the inputs and the returned grids.

voxel_output.npz: n cases; per case k
  name_k            what the case is
  q_k   [2,sH,sW]   int64    the count image (channel 0: positive events, channel 1: negative events)
  bins_k            int64
  vox_k [bins,sH,sW] float32 events_to_voxel_torch(xs, ys, ts, ps, bins, sensor_size=(sH, sW))
Cases: the four count images of event_times.npz with bins 1, 2, 5 and 32 each; two tiny images with N = 3 (all zeros) and N = 4
events; one image whose counts are all 0 or 1 (every time 0.01: dt = 1e-6).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_stubs  # noqa: E402
from event_times_ref import emit_timed_np  # noqa: E402

REF = os.environ.get("BMC_REFERENCE", "/root/reference")
ref_stubs.install()
sys.path.insert(0, REF)
from dataloader.encodings import events_to_voxel_torch  # noqa: E402

BINS = (1, 2, 5, 32)


def cases():
    z = np.load(os.path.join(HERE, "event_times.npz"), allow_pickle=False)
    for k in range(4):
        for bins in BINS:
            yield "event_times_q%d_bins%d" % (k, bins), z["q%d" % k].astype(np.int64), bins
    three = np.zeros((2, 3, 4), np.int64)
    three[0, 1, 2], three[1, 0, 0] = 2, 1
    four = three.copy()
    four[1, 2, 3] = 1
    yield "three_events", three, 5
    yield "four_events", four, 5
    ones = (np.random.default_rng(20261019).random((2, 6, 7)) < 0.4).astype(np.int64)
    yield "counts_0_or_1", ones, 5


def main():
    out, n = {}, 0
    for name, q, bins in cases():
        sH, sW = q.shape[1:]
        xs, ys, ps, ts, _ = emit_timed_np(q.astype(np.float32))
        cols = [torch.from_numpy(v.astype(np.float32)) for v in (xs, ys, ts, ps)]
        vox = events_to_voxel_torch(*cols, bins, sensor_size=(sH, sW))
        assert tuple(vox.shape) == (bins, sH, sW) and vox.dtype == torch.float32
        out["name_%d" % n], out["q_%d" % n], out["bins_%d" % n] = name, q, np.int64(bins)
        out["vox_%d" % n] = vox.numpy().astype(np.float32)
        print(name, q.shape, "events", int(q.sum()), "max count", int(q.max()), "non-zero", int((vox != 0).sum()))
        n += 1
    out["n"] = np.int64(n)
    np.savez_compressed(os.path.join(HERE, "voxel_output.npz"), **out)


if __name__ == "__main__":
    main()
