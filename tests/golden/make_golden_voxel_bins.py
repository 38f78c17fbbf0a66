#!/usr/bin/env python3
"""Golden vectors for the two temporal-bilinear voxel encoders at the bin counts and weights where a fused multiply-add
shows: events_to_voxel (dataloader/encodings.py:272-287) and events_to_voxel_torch (:100-148) of the REFERENCE, run on CPU
tensors, single-threaded so that index_put_(accumulate=True) adds a pixel's events in event order.  Only data is written.

    BMC_REFERENCE=<reference checkout> python tests/golden/make_golden_voxel_bins.py

voxel_bins.npz   "cases": the tags.  Per tag  meta = [H, W, bins],  xs, ys, ts, ps (float32 inputs),  vox [bins,H,W] and
                 xs_after, ys_after (the caller's coordinate tensors after the call).  Tags v_* are events_to_voxel (sub-pixel
                 positions, normalised timestamps), tags t_* events_to_voxel_torch (integer-valued positions, raw timestamps).
                 *_pm<b>: +-1 polarities at b bins (b - 1 no power of two: the product t * (b - 1) is inexact);
                 *_fw<b>, *_wide<b>: float weights (standard normal; normal * 10**uniform(-3, 3));
                 *_centres: timestamps on k / (bins - 1) exactly, with ties;  v_outside: timestamps outside [0, 1];
                 *_alloob: every event outside the sensor;  *_1x1: a one-pixel sensor;  t_norm: normalised timestamps;
                 t_zero_ts, t_three: the two early-outs (all-zero timestamps, <= 3 events).
The archive is written with fixed member dates, so the same inputs give the same bytes."""
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("BMC_REFERENCE")
if not REF:
    sys.exit("set BMC_REFERENCE to a checkout of the reference")
sys.path.insert(0, REF)
from dataloader.encodings import events_to_voxel, events_to_voxel_torch  # noqa: E402

torch.set_num_threads(1)          # sequential index_put_: the summation order of the golden is the event order

# (tag, (H, W), events, bins, weights, timestamps)
SHARED = [("pm4", (5, 7), 200, 4, "pm", "uniform"), ("pm6", (9, 11), 300, 6, "pm", "uniform"),
          ("pm7", (9, 11), 300, 7, "pm", "uniform"), ("pm8", (7, 5), 200, 8, "pm", "uniform"),
          ("pm10", (6, 9), 200, 10, "pm", "uniform"), ("pm11", (3, 4), 150, 11, "pm", "uniform"),
          ("pm33", (5, 7), 200, 33, "pm", "uniform"),
          ("fw2", (5, 7), 200, 2, "normal", "uniform"), ("fw5", (5, 7), 200, 5, "normal", "uniform"),
          ("fw4", (5, 7), 200, 4, "normal", "uniform"), ("fw7", (9, 11), 300, 7, "normal", "uniform"),
          ("wide6", (7, 5), 300, 6, "wide", "uniform"),
          ("centres", (5, 7), 200, 10, "pm", "centres"),
          ("alloob", (4, 6), 300, 23, "normal", "alloob"),
          ("1x1", (1, 1), 400, 23, "normal", "uniform")]
CASES = [("v_" + c[0],) + c[1:] for c in SHARED] + [("v_outside", (5, 7), 200, 6, "normal", "outside")] \
    + [("t_" + c[0],) + c[1:] for c in SHARED] \
    + [("t_norm", (5, 7), 200, 6, "normal", "normalised"), ("t_zero_ts", (5, 7), 50, 7, "normal", "zeros"),
       ("t_three", (5, 7), 3, 7, "normal", "uniform")]


def columns(rng, tag, H, W, n, bins, weights, style):
    torch_variant = tag.startswith("t_")
    if style == "alloob":                            # left of, right of, below and above the sensor; none inside
        side = rng.integers(0, 4, n)
        xs = np.choose(side, [np.full(n, -1.0), np.full(n, W + 0.5), rng.integers(0, W, n) + 0.25, rng.integers(0, W, n) + 0.25])
        ys = np.choose(side, [rng.integers(0, H, n) + 0.5, rng.integers(0, H, n) + 0.5, np.full(n, -0.5), np.full(n, float(H))])
    else:                                            # quarter-pixel positions up to a pixel outside the sensor, its edges included
        xs = rng.integers(-4, 4 * W + 5, n) / 4.0
        ys = rng.integers(-4, 4 * H + 5, n) / 4.0
    if torch_variant:
        xs, ys = np.floor(xs), np.floor(ys)          # integer-valued floats, as events_to_image_torch(interpolation=None) takes
    u = np.sort(rng.uniform(0, 1, n))
    if style == "centres":                           # every timestamp on a bin centre, many ties
        ts = (np.sort(rng.integers(0, bins, n)).astype(np.float32) / np.float32(bins - 1)).astype(np.float32)
    elif style == "outside":                         # (events_to_voxel's caller normalises; the function itself does not care)
        ts = np.sort(rng.uniform(-0.4, 1.4, n)).astype(np.float32)
    elif style == "zeros":
        ts = np.zeros(n, np.float32)
    elif torch_variant and style != "normalised":    # raw sensor time: events_to_voxel_torch normalises by itself
        ts = (1.5 + 0.03 * u).astype(np.float32)
    else:                                            # event_formatting's normalisation (dataloader/base_dataset.py:30)
        ts = u.astype(np.float32)
        ts = ((ts - ts[0]) / (ts[-1] - ts[0] + np.float32(1e-6))).astype(np.float32)
    if weights == "pm":
        ps = rng.choice([-1.0, 1.0], n)
    elif weights == "normal":
        ps = rng.standard_normal(n)
    else:
        ps = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
    return xs.astype(np.float32), ys.astype(np.float32), ts, ps.astype(np.float32)


def main():
    out = {"cases": np.asarray([c[0] for c in CASES])}
    for i, (tag, (H, W), n, bins, weights, style) in enumerate(CASES):
        rng = np.random.default_rng(4200 + i)
        xs, ys, ts, ps = columns(rng, tag, H, W, n, bins, weights, style)
        xt, yt, tt, pt = (torch.tensor(a) for a in (xs, ys, ts, ps))
        fn = events_to_voxel_torch if tag.startswith("t_") else events_to_voxel
        vox = fn(xt, yt, tt, pt, bins, sensor_size=(H, W))
        assert np.array_equal(tt.numpy(), ts) and np.array_equal(pt.numpy(), ps)      # neither function touches ts / ps
        for k, v in (("meta", np.asarray([H, W, bins], np.int64)), ("xs", xs), ("ys", ys), ("ts", ts), ("ps", ps),
                     ("vox", vox.numpy()), ("xs_after", xt.numpy()), ("ys_after", yt.numpy())):
            out["%s/%s" % (tag, k)] = v
    path = os.path.join(HERE, "voxel_bins.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:      # np.savez stamps every member with the clock
        for k, v in out.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.ascontiguousarray(v), allow_pickle=False)
    print("wrote voxel_bins.npz: %d cases, %d bytes" % (len(CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
