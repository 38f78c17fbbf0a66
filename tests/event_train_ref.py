"""numpy restatement of the sequence encoder for training (include/bmc_hip.h "sequence encoder for training"; csrc/seq_encode.hip):
the frames SequenceDataset.__getitem__ (dataloader/h5dataset.py:666-700) returns for a plan, built on
oracle.encode_raw_frame_np.  tests/golden/event_train.npz pins it to the reference; the GPU tests compare the kernel with it."""
import os

import numpy as np

from oracle import bmc_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "event_train.npz")


def lr_frame(cols, rng, flips, size, paused=False, noise=None):
    """One LR item: events [first, end) of the columns with `flips`; the noise events (xs, ys, ps) on top, NOT flipped
    (h5dataset.py:281-285: concatenated after augment_event; every event counts on its own, so the image of the concatenation is
    the sum of the two images); a paused item is all zero, noise included (:304-306)."""
    H, W = size
    if paused:
        return np.zeros((2, H, W), np.float32)
    a, b = int(rng[0]), int(rng[1])
    img = O.encode_raw_frame_np(cols[0][a:b], cols[1][a:b], cols[2][a:b], flips, (H, W))
    if noise is not None and len(noise[0]):
        img = img + O.encode_raw_frame_np(noise[0], noise[1], np.asarray(noise[2], np.float64), 0, (H, W))
    return img


def gt_frame(cols, rng, flips, size):
    """One HR item: the same flips, paused or not, never with noise."""
    a, b = int(rng[0]), int(rng[1])
    return O.encode_raw_frame_np(cols[0][a:b], cols[1][a:b], cols[2][a:b], flips, size)


def encode_sample(lr, gt, lr_ranges, gt_ranges, flips, paused, lr_size, gt_size, noise=None):
    """One sequence -> (inp_cnt [L,2,H,W], gt_cnt [L,2,gh,gw]) float32; lr_ranges / gt_ranges [L,2], paused [L] bools."""
    inp = np.stack([lr_frame(lr, r, flips, lr_size, p, noise) for r, p in zip(lr_ranges, paused)])
    out = np.stack([gt_frame(gt, r, flips, gt_size) for r in gt_ranges])
    return inp, out


def load_golden():
    """-> (g, cases): the npz and per case a dict of its fields and the arguments sequence_plan / EventTrainSet take."""
    g = np.load(GOLDEN)
    cases = {}
    for name in g["cases"].tolist():
        rs, i, L, step, aug, pause, noise = g[name + "_cfg"].tolist()
        cases[name] = dict(
            rs=rs, i=i, L=L, step=None if step < 0 else step,
            augment=(g["mechanisms"].tolist(), g["probs"].tolist()) if aug else None,
            pause=tuple(g[name + "_pause"].tolist()) if pause else None,
            noise_level=float(g[name + "_noise_level"]) if noise else None,
            seed=int(g[name + "_seed"]), items=g[name + "_items"].tolist(), paused=g[name + "_paused"].tolist(),
            flips=int(g[name + "_flips"]), next=float(g[name + "_next"]), inp=g[name + "_inp"].astype(np.float32),
            gt=g[name + "_gt"].astype(np.float32), noise=g[name + "_noise"] if noise else None)
    return g, cases
