#!/usr/bin/env python3
"""Golden training sequences for event_dataset (sequence_plan, noise_events, EventTrainSet.batch): what the REFERENCE's own
SequenceDataset.__getitem__ (dataloader/h5dataset.py:637-700, over H5Dataset.__getitem__ :261-316) returns for one small
synthetic recording read through the stubbed HDF5 file object of ref_stubs.py (build container only: the reference is
imported from BMC_REFERENCE).  Only data is written: the columns, the index tables and the recorded results.

event_train.npz:
  lr_xs / lr_ys / lr_ps, gt_xs / gt_ys / gt_ps      the raw columns (int16, int16, float64); sensor 72x128, LR 9x16, HR 36x64
  lr_index, gt_index [24,2]                         dataset.event_indices / gt_event_indices (window 128 advancing by 64)
  size                                              H, W, gh, gw
  mechanisms, probs, window                         the augmentation list, its probabilities; the LR events per item
  cases                                             the case names; per case c:
    c_cfg      rs, i, L, step (-1: None), augment (0/1), pause (0/1), noise (0/1): random.seed(rs) precedes dataset[i]
    c_pause    proba_pause_when_running, proba_pause_when_paused; c_noise_level
    c_seed     the seed the sequence drew; c_items, c_paused: the (index, Pause) of every H5Dataset.__getitem__ call
    c_flips    which of the three flips augment_event applies for that seed (bit0 H, bit1 V, bit2 P), from a probe event
    c_next     random.random() right after dataset[i]: the state the sampling leaves `random` in
    c_inp [L,2,9,16], c_gt [L,2,36,64]              the items' inp_cnt / gt_cnt as uint8 (they are small integers)
    c_noise [3,n]                                   add_noise_event's x, y, p for that seed (noise cases)
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402

REF = os.environ.get("BMC_REFERENCE", "/root/reference")
ref_stubs.install()
sys.path.insert(0, REF)
from dataloader.h5dataset import H5Dataset, SequenceDataset  # noqa: E402

WINDOW, SLIDING, LENGTH = 128, 64, 24
MECH, PROBS = ["Horizontal", "Vertical", "Polarity"], [0.5, 0.5, 0.5]
PATH = "/fake/event_train.h5"
ref_stubs.FAKE_FILES[PATH] = ref_stubs.synth_nfs_file(91, n_lr=2048, scale=4, sensor=(72, 128), lr_div=8)


def dataset(L, step, augment, pause, noise):
    cfg = {"need_gt_events": True, "scale": 4, "ori_scale": "down8", "time_bins": 1, "mode": "events", "window": WINDOW,
           "sliding_window": SLIDING, "dataset_length": LENGTH,
           "data_augment": {"enabled": bool(augment), "augment": MECH, "augment_prob": PROBS},
           "add_noise": {"enabled": noise is not None, "noise_level": noise if noise is not None else 0.0},
           "sequence": {"sequence_length": L, "step_size": step,
                        "pause": {"enabled": pause is not None, "proba_pause_when_running": pause[0] if pause else 0.0,
                                  "proba_pause_when_paused": pause[1] if pause else 0.0}}}
    return SequenceDataset(PATH, cfg)


def run(sds, rs, i):
    """random.seed(rs); sds[i] -> (sequence, seed, [(index, Pause)], random.random() after)."""
    calls = []
    inner = sds.dataset
    orig = type(inner).__getitem__

    def spy(index, Pause=False, seed=None):
        calls.append((index, bool(Pause), seed))
        return orig(inner, index, Pause=Pause, seed=seed)

    inner.__getitem__ = spy                  # SequenceDataset calls self.dataset.__getitem__(...) by name
    try:
        random.seed(rs)
        seq = sds[i]
        nxt = random.random()
    finally:
        del inner.__getitem__
    assert len({c[2] for c in calls}) == 1
    return seq, calls[0][2], [(c[0], c[1]) for c in calls], nxt


def flips_of(ds, seed):
    """Which flips the reference's augment_event applies for this seed, read off a probe event (x, y, t, p) = (1, 2, 0, 1)."""
    state = random.getstate()
    ev = ds.augment_event(np.asarray([[1.0], [2.0], [0.0], [1.0]]), ds.inp_sensor_resolution, seed)
    random.setstate(state)
    return int(ev[0, 0] != 1.0) | int(ev[1, 0] != 2.0) << 1 | int(ev[3, 0] != 1.0) << 2


# name: L, step, augment, pause, noise level, sequence index, and what the searched random.seed must give
CASES = {
    "plain":     dict(L=5, step=None, augment=0, pause=None, noise=None, i=1, want=lambda f, p: True),
    "step3":     dict(L=5, step=3, augment=0, pause=None, noise=None, i=4, want=lambda f, p: True),
    "flips_all": dict(L=4, step=3, augment=1, pause=None, noise=0.1, i=2, want=lambda f, p: f == 7),
    "flips_none": dict(L=4, step=None, augment=1, pause=None, noise=None, i=3, want=lambda f, p: f == 0),
    "flips_some": dict(L=5, step=3, augment=1, pause=None, noise=None, i=0, want=lambda f, p: f in (1, 2, 3, 4, 5, 6)),
    "pause":     dict(L=6, step=None, augment=0, pause=(0.4, 0.6), noise=None, i=2,
                      want=lambda f, p: sum(p) >= 2 and not p[-1] and any(a and b for a, b in zip(p, p[1:]))),
    "pause_noise": dict(L=5, step=3, augment=0, pause=(0.5, 0.5), noise=0.25, i=5, want=lambda f, p: p[-1] and not p[1]),
    # augmentation re-seeds `random` in every item: all pause draws are ONE number u.  0.3 <= u < 0.6: paused, running, ...
    "pause_degenerate": dict(L=6, step=3, augment=1, pause=(0.6, 0.3), noise=0.1, i=1,
                             want=lambda f, p: p == [False, True, False, True, False, True]),
    "pause_degenerate_all": dict(L=4, step=None, augment=1, pause=(0.9, 0.9), noise=None, i=0,
                                 want=lambda f, p: p == [False, True, True, True]),
}

out = {}
st = ref_stubs.FAKE_FILES[PATH]
for side, prex in (("lr", "down8"), ("gt", "down2")):
    for c in ("xs", "ys", "ps"):
        out["%s_%s" % (side, c)] = st["%s_events/%s" % (prex, c)]
seen_paused = seen_all = seen_none = False
for name, c in CASES.items():
    sds = dataset(c["L"], c["step"], c["augment"], c["pause"], c["noise"])
    ds = sds.dataset
    assert ds.length == LENGTH and len(ds.gt_event_indices) >= LENGTH
    assert list(ds.inp_sensor_resolution) == [9, 16] and list(ds.gt_sensor_resolution) == [36, 64]
    for rs in range(1000):
        seq, seed, calls, nxt = run(sds, rs, c["i"])
        flips = flips_of(ds, seed) if c["augment"] else 0
        if c["want"](flips, [p for _, p in calls]):
            break
    else:
        raise SystemExit("no seed found for " + name)
    assert len(seq) == c["L"] == len(calls)
    inp = np.stack([it["inp_cnt"].numpy() for it in seq])
    gt = np.stack([it["gt_cnt"].numpy() for it in seq])
    for a in (inp, gt):
        assert a.dtype == np.float32 and (a == np.round(a)).all() and a.min() >= 0 and a.max() <= 255
    paused = [p for _, p in calls]
    seen_paused |= any(paused)
    seen_all |= flips == 7
    seen_none |= bool(c["augment"]) and flips == 0
    for t, p in enumerate(paused):
        assert not p or not inp[t].any()
    out[name + "_cfg"] = np.asarray([rs, c["i"], c["L"], -1 if c["step"] is None else c["step"], c["augment"],
                                     int(c["pause"] is not None), int(c["noise"] is not None)], np.int64)
    out[name + "_pause"] = np.asarray(c["pause"] or (0.0, 0.0), np.float64)
    out[name + "_noise_level"] = np.asarray(c["noise"] or 0.0, np.float64)
    out[name + "_seed"] = np.asarray(seed, np.int64)
    out[name + "_items"] = np.asarray([j for j, _ in calls], np.int64)
    out[name + "_paused"] = np.asarray(paused, np.bool_)
    out[name + "_flips"] = np.asarray(flips, np.int64)
    out[name + "_next"] = np.asarray(nxt, np.float64)
    out[name + "_inp"] = inp.astype(np.uint8)
    out[name + "_gt"] = gt.astype(np.uint8)
    if c["noise"] is not None:
        noise = H5Dataset.add_noise_event(WINDOW, ds.inp_sensor_resolution, seed, noise_level=c["noise"]).numpy()
        assert noise.shape[0] == 4 and (noise[2] == 1).all()
        out[name + "_noise"] = noise[[0, 1, 3]].astype(np.int16)
    print(name, "rs", rs, "seed", seed, "flips", flips, "items", [j for j, _ in calls], "paused", [int(p) for p in paused])
assert seen_paused and seen_all and seen_none
out["lr_index"] = np.asarray(ds.event_indices, np.int64)[:LENGTH]
out["gt_index"] = np.asarray(ds.gt_event_indices, np.int64)[:LENGTH]
out["size"] = np.asarray([9, 16, 36, 64])
out["mechanisms"] = np.asarray(MECH)
out["probs"] = np.asarray(PROBS)
out["window"] = np.asarray(WINDOW)
out["cases"] = np.asarray(list(CASES))
path = os.path.join(HERE, "event_train.npz")
np.savez_compressed(path, **out)
print("wrote event_train.npz: %d bytes" % os.path.getsize(path))
