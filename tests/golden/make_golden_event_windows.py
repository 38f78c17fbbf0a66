#!/usr/bin/env python3
"""Golden index tables for bmc_hip.encodings.event_window_indices: the event blocks the REFERENCE's own H5Dataset cuts three
small synthetic recordings into (mode 'events': dataloader/h5dataset.py set_data_mode :164-195, compute_k_indices :197-215,
get_gt_event_indices_num :362-390), read through the stubbed HDF5 file object of ref_stubs.py (build container only: the
reference is imported from BMC_REFERENCE).  Only data is written: the columns and the tables.

event_windows.npz, per recording r in (a, b, c):
  r_lr_xs / r_lr_ys / r_lr_ps / r_lr_ts, r_gt_*   the columns (int16, int16, float64, float64)
  r_cfg                                           window, sliding_window, scale, dataset_length (-1: None)
  r_size                                          H, W, gh, gw
  r_lr_index, r_gt_index                          dataset.event_indices / dataset.gt_event_indices
a: window 256 / sliding 128, its last two LR blocks are clamped to num_events - 1; runs of duplicate timestamps in both
   streams, in the LR stream exactly at the block starts;
b: window 64 / sliding 48 (blocks advance by 16), HR blocks of 1 024 out of 1 500 events: most are moved back to end at
   num_gt_events - 1; a run of 18 equal LR timestamps covers two block starts (both ask for the same HR event: the second
   gets the next one); dataset_length caps the table below its natural length;
c: as b, but the HR stream ends at t = 0.6: the reference finds no HR block for the LR blocks that start later, its
   gt_event_indices is SHORTER than event_indices (item access fails there).
(The `gt_idx0 < 0` clamp of get_gt_event_indices_num cannot fire: the search returns no negative index.)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402

REF = os.environ.get("BMC_REFERENCE", "/root/reference")
ref_stubs.install()
sys.path.insert(0, REF)
from dataloader.h5dataset import H5Dataset  # noqa: E402


def columns(rng, n, h, w, t_end, dup_every, run=None):
    xs = rng.integers(0, w, n).astype(np.int16)
    ys = rng.integers(0, h, n).astype(np.int16)
    bad = rng.integers(0, n, max(n // 100, 2))
    xs[bad[::2]] = w + rng.integers(0, 2, bad[::2].size)
    ys[bad[1::2]] = -1 - rng.integers(0, 2, bad[1::2].size)
    ts = np.sort(rng.uniform(0.0, t_end, n))
    for k in range(0, n - 4, dup_every):                      # runs of equal timestamps
        ts[k:k + 3] = ts[k]
    if run is not None:
        ts[run[0]:run[1]] = ts[run[0]]
    return xs, ys, np.sort(ts), rng.choice([-1.0, 1.0], n)


def recording(tag, seed, n_lr, n_gt, lr_hw, window, sliding, scale, dataset_length, gt_t_end, dup_lr, dup_gt, run=None):
    rng = np.random.default_rng(seed)
    H, W = lr_hw
    gh, gw = H * scale, W * scale
    lr = columns(rng, n_lr, H, W, 1.0, dup_lr, run)
    gt = columns(rng, n_gt, gh, gw, gt_t_end, dup_gt)
    # sensor_resolution is the full-size sensor: LR = down8, ground truth = down(8 / scale)
    store = {"attrs": {"sensor_resolution": np.asarray([H * 8, W * 8])}}
    for prex, (xs, ys, ts, ps) in (("down8", lr), ("down%d" % (8 // scale), gt)):
        for name, col in (("xs", xs), ("ys", ys), ("ts", ts), ("ps", ps)):
            store["%s_events/%s" % (prex, name)] = col
    path = "/fake/%s.h5" % tag
    ref_stubs.FAKE_FILES[path] = store
    cfg = {"need_gt_events": True, "scale": scale, "ori_scale": "down8", "time_bins": 1, "mode": "events", "window": window,
           "sliding_window": sliding, "data_augment": {"enabled": False}}
    if dataset_length is not None:
        cfg["dataset_length"] = dataset_length
    ds = H5Dataset(path, cfg)
    assert list(ds.inp_sensor_resolution) == [H, W] and list(ds.gt_sensor_resolution) == [gh, gw]
    out = {tag + "_cfg": np.asarray([window, sliding, scale, -1 if dataset_length is None else dataset_length]),
           tag + "_size": np.asarray([H, W, gh, gw]),
           tag + "_lr_index": np.asarray(ds.event_indices, np.int64), tag + "_gt_index": np.asarray(ds.gt_event_indices, np.int64)}
    for side, (xs, ys, ts, ps) in (("lr", lr), ("gt", gt)):
        out.update({"%s_%s_xs" % (tag, side): xs, "%s_%s_ys" % (tag, side): ys, "%s_%s_ts" % (tag, side): ts,
                    "%s_%s_ps" % (tag, side): ps})
    for j in range(len(ds.gt_event_indices)):                  # every item of the table is one the reference can read
        ds.get_event_indices(j), ds.get_gt_event_indices(j)
    return out


out = {}
out.update(recording("a", 71, n_lr=1024, n_gt=1024 * 4, lr_hw=(10, 16), window=256, sliding=128, scale=2, dataset_length=None,
                     gt_t_end=1.0, dup_lr=128, dup_gt=37))
out.update(recording("b", 72, n_lr=400, n_gt=1500, lr_hw=(6, 8), window=64, sliding=48, scale=4, dataset_length=20,
                     gt_t_end=1.0, dup_lr=16, dup_gt=11, run=(32, 50)))
out.update(recording("c", 73, n_lr=400, n_gt=1500, lr_hw=(6, 8), window=64, sliding=48, scale=4, dataset_length=None,
                     gt_t_end=0.6, dup_lr=16, dup_gt=11))
np.savez_compressed(os.path.join(HERE, "event_windows.npz"), **out)
print("wrote event_windows.npz:", {k: v.shape for k, v in out.items()})
for t in "abc":
    print(t, "lr", out[t + "_lr_index"][:3].tolist(), "...", out[t + "_lr_index"][-3:].tolist())
    print(t, "gt", out[t + "_gt_index"][:3].tolist(), "...", out[t + "_gt_index"][-3:].tolist())
