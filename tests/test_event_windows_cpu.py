"""CPU checks of event-backed multi-stream inference (infer.MultiStreamSR.open_events, csrc/slot_events.hip): the index
tables of bmc_hip.encodings.event_window_indices against tables recorded from the reference's own H5Dataset
(tests/golden/event_windows.npz, written by tests/golden/make_golden_event_windows.py), open_events' argument checks, the
layout of bmc_slot_events_t, and the gfx950 code of the encode kernel (no flat memory instructions, no scratch)."""
import os
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


def _golden():
    return np.load(os.path.join(HERE, "golden", "event_windows.npz"))


def _tables(z, tag):
    from bmc_hip.encodings import event_window_indices
    window, sliding, scale, length = (int(v) for v in z[tag + "_cfg"])
    return event_window_indices(z[tag + "_lr_ts"], z[tag + "_gt_ts"], window=window, sliding_window=sliding, scale=scale,
                                dataset_length=None if length < 0 else length)


# ------------------------------------------------------------------ index tables
@pytest.mark.parametrize("tag", ["a", "b"])
def test_index_tables_equal_the_reference_dataset(tag):
    """a: the tail LR blocks are clamped to num_events - 1; b: HR blocks moved back to end at num_gt_events - 1, two blocks
    that start on one timestamp, dataset_length; duplicate timestamps in both."""
    z = _golden()
    lr_index, gt_index = _tables(z, tag)
    assert lr_index.dtype == np.int64 and gt_index.dtype == np.int64
    assert np.array_equal(lr_index, z[tag + "_lr_index"])
    assert np.array_equal(gt_index, z[tag + "_gt_index"])


def test_golden_recordings_exercise_the_quirks():
    z = _golden()
    a, b = z["a_lr_index"], z["b_lr_index"]
    assert (a[-2:, 1] == len(z["a_lr_ts"]) - 1).all() and a[-1, 1] - a[-1, 0] < a[0, 1] - a[0, 0]        # clamped tail blocks
    g = z["b_gt_index"]
    assert (g[-3:, 1] == len(z["b_gt_ts"]) - 1).all() and (g[:, 1] - g[:, 0] == 16 * (b[0, 1] - b[0, 0])).all()
    ts = z["b_lr_ts"]
    assert ts[b[2, 0]] == ts[b[3, 0]] and g[3, 0] == g[2, 0] + 1                # one timestamp, two block starts: the next HR event
    assert len(b) == 20 < len(ts) // 16                                         # dataset_length caps the table
    for t in "ab":
        for side in ("lr", "gt"):
            assert (np.diff(z["%s_%s_ts" % (t, side)]) == 0).any()              # duplicate timestamps


def test_blocks_without_ground_truth_end_the_tables():
    """c: the HR stream ends before the LR stream.  The reference's gt_event_indices is shorter than its event_indices (item
    access fails beyond it); both tables end there."""
    z = _golden()
    lr_index, gt_index = _tables(z, "c")
    n = len(z["c_gt_index"])
    assert n < len(z["c_lr_index"]) and len(lr_index) == len(gt_index) == n
    assert np.array_equal(lr_index, z["c_lr_index"][:n]) and np.array_equal(gt_index, z["c_gt_index"])


@pytest.mark.parametrize("mode", ["time", "frame", "voxel"])
def test_other_modes_raise(mode):
    from bmc_hip.encodings import event_window_indices
    z = _golden()
    with pytest.raises(ValueError):
        event_window_indices(z["a_lr_ts"], z["a_gt_ts"], 256, 128, 2, mode=mode)


def test_too_few_events_raise():
    from bmc_hip.encodings import event_window_indices
    with pytest.raises(ValueError):
        event_window_indices(np.linspace(0, 1, 100), np.linspace(0, 1, 1600))


# ------------------------------------------------------------------ open_events: argument checks (no device needed)
def _session(seqn=3):
    from infer import MultiStreamSR
    return MultiStreamSR(torch.nn.Identity(), 2, n_c=16, scale=4, seqn=seqn)


def _columns(n, dt=(torch.int16, torch.int16, torch.float64)):
    return tuple(torch.ones(n).to(d) for d in dt)


def _good(L=4, n_lr=100, n_gt=400):
    lr_index = np.stack([20 * np.arange(L), 20 * np.arange(L) + 40], 1)
    gt_index = np.stack([80 * np.arange(L), 80 * np.arange(L) + 160], 1)
    return dict(lr=_columns(n_lr), gt=_columns(n_gt), lr_index=lr_index, gt_index=gt_index, lr_size=(10, 16), gt_size=(40, 64))


def test_open_events_needs_gpu_columns():
    """Everything that can be checked on the host passes; the columns themselves must live on the GPU."""
    with pytest.raises(ValueError, match="GPU"):
        _session().open_events(**_good())


@pytest.mark.parametrize("case,match", [
    ("lr_beyond", "outside"), ("gt_beyond", "outside"), ("negative", "outside"), ("reversed", "first > end"),
    ("lr_dtype", "int16, int16, float64"), ("ps_dtype", "int16, int16, float64"), ("lengths", "one length"),
    ("rows", "rows"), ("float_table", "integer"), ("shape", "integer"), ("short", "fewer than one window"),
    ("two_columns", "three tensors"), ("wide", "wide"), ("size", "lr_size"),
])
def test_open_events_refuses_bad_arguments(case, match):
    a = _good()
    if case == "lr_beyond":
        a["lr_index"][-1, 1] = 101
    elif case == "gt_beyond":
        a["gt_index"][1, 1] = 401
    elif case == "negative":
        a["gt_index"][0, 0] = -1
    elif case == "reversed":
        a["lr_index"][2] = (50, 49)
    elif case == "lr_dtype":
        a["lr"] = _columns(100, (torch.int32, torch.int16, torch.float64))
    elif case == "ps_dtype":
        a["gt"] = _columns(400, (torch.int16, torch.int16, torch.float32))
    elif case == "lengths":
        a["lr"] = a["lr"][:2] + (torch.ones(99, dtype=torch.float64),)
    elif case == "rows":
        a["gt_index"] = a["gt_index"][:-1]
    elif case == "float_table":
        a["lr_index"] = a["lr_index"].astype(np.float64)
    elif case == "shape":
        a["lr_index"] = a["lr_index"].reshape(-1)
    elif case == "short":
        a["lr_index"], a["gt_index"] = a["lr_index"][:2], a["gt_index"][:2]
    elif case == "two_columns":
        a["lr"] = a["lr"][:2]
    elif case == "wide":
        a["gt_size"] = (40, 7681)
    elif case == "size":
        a["lr_size"] = (10,)
    ms = _session()
    with pytest.raises(ValueError, match=match):
        ms.open_events(**a)
    assert not ms.sched.pending() and ms._size is None          # nothing was queued


def test_open_events_limits_seqn():
    with pytest.raises(ValueError, match="seqn"):
        _session(seqn=9).open_events(**_good(L=12, n_lr=400, n_gt=1600))


def test_event_recording_fields():
    from infer import EventRecording
    assert EventRecording._fields == ("lr", "gt", "lr_index", "gt_index", "lr_size", "gt_size")


# ------------------------------------------------------------------ C ABI
def test_library_exports_slot_encode():
    from bmc_hip import lib
    assert "bmc_slot_encode" in lib.EXPORTS and lib.has_symbol("bmc_slot_encode")


def test_slot_events_struct_layout_matches_header():
    import abi_ref
    from bmc_hip import slots
    structs, constants = abi_ref.compiled_header()
    size, compiled = structs["bmc_slot_events_t"]
    dt = slots.SLOT_EVENTS_DTYPE
    assert [size, compiled["gt_xs"][0], compiled["gt_range"][0], compiled["lr_range"][0], constants["BMC_SLOT_MAX_SEQN"],
            structs["bmc_slot_t"][0]] == [dt.itemsize, dt.fields["gt_xs"][1], dt.fields["gt_range"][1], dt.fields["lr_range"][1],
                                          slots.MAX_SEQN, slots.SLOT_DTYPE.itemsize]
    assert dt.fields["lr_range"][0].shape == (slots.MAX_SEQN, 2)


# ------------------------------------------------------------------ ISA of csrc/slot_events.hip
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_encode_kernel_has_no_flat_memory_instructions_and_no_scratch(tmp_path):
    from test_isa_hygiene import CSRC, _kernels
    o = os.path.join(tmp_path, "slot_events.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", o, os.path.join(CSRC, "slot_events.hip")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    ks = {n: k for n, k in _kernels(o).items() if "NumVgprs" in k}
    assert len(ks) == 1 and "slot_encode_kernel" in next(iter(ks)), sorted(ks)
    (k,) = ks.values()
    assert k["flat"] == 0 and k["ScratchSize"] == 0, k
    text = open(o).read()
    assert "global_atomic" not in text and "ds_add_u32" in text      # counts are LDS integer atomics, nothing atomic on global memory
