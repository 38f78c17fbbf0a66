#!/usr/bin/env python
"""hot_filter.npz: inputs and outputs of the REFERENCE's get_hot_event_mask (dataloader/encodings.py:349-364), imported from the
reference checkout named by the environment variable BMC_REFERENCE (build container only; only the data is committed).

Per case k: rate_k (float32 [H,W], the input), params_k (float64 [4]: idx, max_px, min_obvs, max_rate), mask_k (the returned
mask) and after_k (event_rate after the call: the selected entries are zeroed in place).  Sizes <= 12x16.  The cases cover ties,
more candidates than max_px, the float32 boundary of 0.8 (4/5), both sides of idx > min_obvs, NaN, -0.0, +-inf, max_px = 0,
negative max_rate, and random count images.  The script also repeats the check of the contract's integer form (tests/
hot_filter_ref.py::mask_from_counts_np) against the reference's function on 400 random count images."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = os.environ.get("BMC_REFERENCE")
if not REF:
    sys.exit("set BMC_REFERENCE to the reference checkout")
sys.path.insert(0, REF)
from dataloader.encodings import get_hot_event_mask  # noqa: E402

from hot_filter_ref import mask_from_counts_np  # noqa: E402


def run(rate, idx, max_px, min_obvs, max_rate):
    t = torch.from_numpy(np.array(rate, np.float32, copy=True))
    mask = get_hot_event_mask(t, idx, max_px=max_px, min_obvs=min_obvs, max_rate=max_rate)
    return mask.numpy().astype(np.float32), t.numpy()


def cases(rng):
    def counts(H, W, idx, p_hot=0.1):
        c = rng.binomial(idx, 0.2, (H, W))
        hot = rng.random((H, W)) < p_hot
        return np.where(hot, rng.integers(max(idx - 2, 0), idx + 1, (H, W)), c)

    for H, W in ((5, 7), (12, 16), (1, 9)):
        for idx, max_px, min_obvs, max_rate in ((10, 3, 5, 0.8), (10, 100, 5, 0.8), (6, 2, 5, 0.5), (5, 100, 5, 0.1),
                                                (6, 100, 6, 0.1), (7, 100, 6, 0.1), (20, 0, 5, 0.5), (8, 4, 0, 0.0),
                                                (8, 1000, 0, -0.5), (8, 3, 0, -0.5), (9, 5, 2, 1.0), (300, 7, 5, 0.25)):
            c = counts(H, W, idx)
            yield (c.astype(np.float32) / np.float32(idx)), idx, max_px, min_obvs, max_rate
    # the float32 boundary: float32(4) / float32(5) > 0.8 is False, 5/5 is above
    yield np.array([[4, 5, 4], [3, 4, 5]], np.float32) / np.float32(5), 5, 100, 2, 0.8
    yield np.array([[8, 10, 9], [7, 8, 10]], np.float32) / np.float32(10), 10, 100, 2, 0.8
    # ties everywhere: the first max_px in flat order
    yield np.ones((4, 6), np.float32), 9, 5, 1, 0.5
    yield np.ones((12, 16), np.float32), 9, 100, 1, 0.5
    # special values
    a = rng.random((6, 8)).astype(np.float32)
    b = a.copy(); b[3, 2] = np.nan
    yield b, 9, 100, 1, 0.1
    b = a.copy(); b[0, 0] = np.nan
    yield b, 9, 100, 1, 0.1
    b = a.copy(); b[1, 1] = np.inf; b[2, 2] = -np.inf; b[0, 3] = -0.0
    yield b, 9, 5, 1, 0.5
    yield b, 9, 100, 1, -0.25
    b = (a - 0.5).astype(np.float32); b[2, 5] = -0.0; b[4, 1] = 0.0
    yield b, 9, 100, 1, -0.25
    yield b, 9, 3, 1, -0.25
    yield b, 9, 100, 1, 0.0
    yield (-a - 0.1).astype(np.float32), 9, 100, 1, -0.5          # every entry negative, some above max_rate
    yield (-a - 0.1).astype(np.float32), 9, 100, 1, -5.0
    yield (-a - 1.0).astype(np.float32), 9, 100, 1, -0.5          # every entry below max_rate
    z = np.zeros((3, 5), np.float32); z[0, 0] = -0.0; z[2, 4] = 0.7
    yield z, 9, 100, 1, -0.5
    yield z, 9, 1, 1, -0.5
    yield np.full((3, 4), -0.0, np.float32), 9, 100, 1, -0.5


def main():
    rng = np.random.default_rng(20261017)
    out = {}
    k = 0
    for rate, idx, max_px, min_obvs, max_rate in cases(rng):
        mask, after = run(rate, idx, max_px, min_obvs, max_rate)
        out["rate_%d" % k] = np.asarray(rate, np.float32)
        out["params_%d" % k] = np.array([idx, max_px, min_obvs, max_rate], np.float64)
        out["mask_%d" % k], out["after_%d" % k] = mask, after
        k += 1
    out["n"] = np.array(k)
    np.savez_compressed(os.path.join(HERE, "hot_filter.npz"), **out)
    # the integer form of the contract against the reference's function
    bad = over = 0
    for _ in range(400):
        H, W = int(rng.integers(1, 13)), int(rng.integers(1, 17))
        idx = int(rng.integers(1, 40))
        max_px, min_obvs = int(rng.integers(0, 12)), int(rng.integers(0, 8))
        max_rate = float(rng.choice([0.0, 0.25, 0.5, 0.8, 1.0, -0.5, rng.random()]))
        c = rng.integers(0, idx + 1, (H, W))
        mask, _ = run(c.astype(np.float32) / np.float32(idx), idx, max_px, min_obvs, max_rate)
        mine = mask_from_counts_np(c, idx, max_px, min_obvs, max_rate)
        bad += not np.array_equal(mask.astype(np.uint8), mine)
        over += int((mine == 0).sum() == max_px and max_px > 0)
    print("%d cases written; integer form: 400 random cases, %d at the max_px limit, %d mismatches" % (k, over, bad))
    assert bad == 0


if __name__ == "__main__":
    main()
