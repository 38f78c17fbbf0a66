#!/usr/bin/env python3
"""Golden event clouds for the timed event output (include/bmc_hip.h, bmc_slot_emit_timed): what the REFERENCE's own
python_event_redistribute_PolarityStack(mode='linear') (dataloader/encodings.py:367-414) returns for four small quantised
count images (build container only: the reference is imported from BMC_REFERENCE; it ran unpatched under the installed
torch).  Only data is written: the inputs and the returned clouds.

event_times.npz, per image k in 0 .. 3:
  q{k}      [2,sH,sW] int64   the count image (channel 0: positive events, channel 1: negative events)
  cloud{k}  [N,4] float32     the reference's cloud [x, row, t, p] for the stack [1,2,1,sH,sW] = (q[0], -q[1]) -- channel 1
                              negated, so that the reference's sign rule gives p = -1 there; sorted by t with Python's sorted()
Images: 0: 9x12, small counts (1, 2, 3, 5 and their many ties: 1/2 = 2/4, every j = 0, every j = n-1); 1: 7x9 with counts
above 30 (31, 33, 47, 64, 101, 128, 255) among small ones; 2: 6x8, every element but one 3 (three tie groups); 3: 5x6, one
event per element but one (every time equal).  A few hundred to about two thousand events each: the reference sorts a Python list of tensors.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402

REF = os.environ.get("BMC_REFERENCE", "/root/reference")
ref_stubs.install()
sys.path.insert(0, REF)
from dataloader.encodings import python_event_redistribute_PolarityStack  # noqa: E402


def images():
    rng = np.random.default_rng(20261017)
    a = rng.choice([0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 5, 7, 9], (2, 9, 12))
    b = rng.choice([0, 0, 0, 0, 1, 2, 3, 5], (2, 7, 9))
    big = [31, 47, 64, 101, 255, 33, 128]
    for k, v in enumerate(big):
        b[k % 2, (3 * k) % 7, (5 * k + 1) % 9] = v
    c, d = np.full((2, 6, 8), 3), np.ones((2, 5, 6), np.int64)
    c[1, 0, 0] = d[1, 0, 0] = 0          # the reference returns an empty cloud when the SIGNED stack sums to zero (:381)
    return [a, b, c, d]


def main():
    out = {}
    for k, q in enumerate(images()):
        q = q.astype(np.int64)
        stack = torch.tensor(np.stack([q[0], -q[1]]).astype(np.float32))[None, :, None]      # [1,2,1,sH,sW]
        cloud = python_event_redistribute_PolarityStack(stack, mode='linear')
        assert cloud.shape == (1, int(q.sum()), 4), (cloud.shape, q.sum())
        out["q%d" % k], out["cloud%d" % k] = q, cloud[0].numpy().astype(np.float32)
        print("image", k, q.shape, "events", int(q.sum()), "max count", int(q.max()))
    np.savez_compressed(os.path.join(HERE, "event_times.npz"), **out)


if __name__ == "__main__":
    main()
