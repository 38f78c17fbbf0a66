"""CPU checks of the event output of multi-stream inference (infer.MultiStreamSR(emit_events=True), csrc/slot_emit.hip): the
definition of the emitted stream (event_output_ref.emit_np) round-trips through the oracle's encoder on the reference's own
predictions, the argument checks of the public entry points, the layout of bmc_slot_emit_t, the export, and the gfx950 code
of the two emit kernels (no flat memory instructions, no scratch, no atomics on global memory, nothing that waits)."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from event_output_ref import counts_np, emit_np, quantise_np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------ the definition
def test_restatement_round_trips_through_the_oracle_encoder_on_the_golden_predictions():
    """Every prediction of infer_seqn3.npz: encoding its emitted events with flags 0 at (sH, sW) gives q exactly; the golden
    is not a trivial case (thousands of events, counts above 1, both polarities)."""
    from oracle import bmc_oracle as O
    z = np.load(os.path.join(HERE, "golden", "infer_seqn3.npz"))
    scale, n_c, n_b, B, H, W, seqn, nwin, gh, gw = (int(v) for v in z["meta"])
    seen = 0
    for i in range(nwin):
        for b in range(B):
            P = z["pred%d" % i][b]
            xs, ys, ps, q = emit_np(P)
            assert P.shape == (2, scale * H, scale * W) and len(xs) == len(ys) == len(ps) == q.sum()
            assert len(xs) >= 2000 and q.max() >= 2 and (ps < 0).sum() >= 500 and (q > 0).mean() >= 0.4
            assert xs.min() >= 0 and xs.max() < scale * W and ys.min() >= 0 and ys.max() < scale * H
            img = O.encode_raw_frame_np(xs, ys, ps.astype(np.float64), 0, (scale * H, scale * W))
            assert np.array_equal(img, q.astype(img.dtype))
            assert np.array_equal(counts_np(xs, ys, ps, scale * H, scale * W), q)
            seen += 1
    assert seen == 8


def test_quantisation_rule():
    v = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -0.0, 0.0, np.nan, np.inf, -np.inf, 300.0, 254.5, 255.5, 0.49999997, 0.50000006,
                  1e-30, -3.0], np.float32)
    assert quantise_np(v).tolist() == [0, 2, 2, 4, 0, 0, 0, 0, 255, 0, 255, 254, 255, 0, 1, 0, 0]
    assert quantise_np(v, 2).tolist() == [0, 2, 2, 2, 0, 0, 0, 0, 2, 0, 2, 2, 2, 0, 1, 0, 0]
    xs, ys, ps, q = emit_np(np.array([[[0.0, 2.0], [1.0, 0.0]], [[0.0, 0.0], [0.0, 3.0]]], np.float32))
    assert xs.tolist() == [1, 1, 0, 1, 1, 1] and ys.tolist() == [1, 1, 0, 0, 0, 0] and ps.tolist() == [1, 1, 1, -1, -1, -1]


# ------------------------------------------------------------------ argument checks (no device needed)
def _session(**kw):
    from infer import MultiStreamSR
    return MultiStreamSR(torch.nn.Identity(), 2, n_c=16, scale=4, **kw)


@pytest.mark.parametrize("bad", [0, -1, 32768, 2.5, None, True])
def test_session_refuses_bad_max_count(bad):
    with pytest.raises(ValueError, match="max_count"):
        _session(emit_events=True, max_count=bad)


def test_session_defaults():
    ms = _session()
    assert ms.emit_events is False and ms.max_count == 255
    assert _session(emit_events=True, max_count=32767).max_count == 32767


def _frames():
    return torch.zeros(4, 2, 10, 16), torch.zeros(4, 2, 40, 64)


def _event_args():
    cols = lambda n: (torch.ones(n, dtype=torch.int16), torch.ones(n, dtype=torch.int16), torch.ones(n, dtype=torch.float64))
    lr_index = np.stack([20 * np.arange(4), 20 * np.arange(4) + 40], 1)
    gt_index = np.stack([80 * np.arange(4), 80 * np.arange(4) + 160], 1)
    return dict(lr=cols(100), gt=cols(400), lr_index=lr_index, gt_index=gt_index, lr_size=(10, 16), gt_size=(40, 64))


@pytest.mark.parametrize("kind", ["open", "open_events"])
def test_event_capacity_needs_an_emitting_session(kind):
    ms = _session()
    with pytest.raises(ValueError, match="emit_events=True"):
        ms.open(*_frames(), event_capacity=100) if kind == "open" else ms.open_events(event_capacity=100, **_event_args())
    assert not ms.sched.pending() and ms._size is None


@pytest.mark.parametrize("kind", ["open", "open_events"])
@pytest.mark.parametrize("bad", [0, -5, 1.5, "many", True])
def test_event_capacity_must_be_a_positive_integer(kind, bad):
    ms = _session(emit_events=True)
    with pytest.raises(ValueError, match="positive integer"):
        ms.open(*_frames(), event_capacity=bad) if kind == "open" else ms.open_events(event_capacity=bad, **_event_args())
    assert not ms.sched.pending() and ms._size is None


def test_open_still_needs_gpu_tensors_when_emitting():
    """A good capacity passes the host checks; the recording itself must live on the GPU (no CPU path)."""
    ms = _session(emit_events=True)
    with pytest.raises(ValueError, match="GPU"):
        ms.open(*_frames(), event_capacity=1000)
    with pytest.raises(ValueError, match="GPU"):
        ms.open_events(event_capacity=1000, **_event_args())


def test_open_refuses_predictions_too_large_for_int16_coordinates():
    from infer import MultiStreamSR
    ms = MultiStreamSR(torch.nn.Identity(), 2, n_c=16, scale=4, emit_events=True)
    a = _event_args()
    a["lr_size"], a["gt_size"] = (10, 7000), (40, 7000)              # 4 x 7000 = 28 000 fits: only the device is missing
    with pytest.raises(ValueError, match="GPU"):
        ms.open_events(**a)
    ms = MultiStreamSR(torch.nn.Identity(), 2, n_c=16, scale=8, emit_events=True)
    a["lr_size"] = (10, 4096)                                         # 8 x 4096 = 32 768 > 32 767
    with pytest.raises(ValueError, match="int16"):
        ms.open_events(**a)


def test_slots_emit_refusals():
    from bmc_hip import slots
    pred = torch.zeros(2, 2, 8, 8)
    parts = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="no emit entries"):
        slots.emit(types.SimpleNamespace(S=2, emit=False), pred, 255, 1, parts)
    table = types.SimpleNamespace(S=2, emit=True, timed=False)
    for bad in (0, 32768, 1.0):
        with pytest.raises(ValueError, match="max_count"):
            slots.emit(table, pred, bad, 1, parts)
    for bad in (0, slots.MAX_EMIT_PARTS + 1):
        with pytest.raises(ValueError, match="nparts"):
            slots.emit(table, pred, 255, bad, parts)
    with pytest.raises(ValueError, match="GPU tensor"):
        slots.emit(table, pred, 255, 1, parts)                        # a CPU tensor: there is no CPU path
    assert slots.EMIT_LAUNCHES == 0


def test_emit_parts():
    from bmc_hip import slots
    assert slots.emit_parts(36, 56) == 1 and slots.emit_parts(124, 224) == 14
    assert slots.emit_parts(720, 960) == 338 > 256                    # more workgroups per slot than the chip has CUs
    assert slots.emit_parts(32767, 32767) == slots.MAX_EMIT_PARTS == 1024


def test_counts_to_events_refusals():
    from bmc_hip.encodings import counts_to_events
    with pytest.raises(ValueError, match=r"\[B,2,sH,sW\]"):
        counts_to_events(torch.zeros(2, 3, 8, 8))
    with pytest.raises(ValueError, match="max_count"):
        counts_to_events(torch.zeros(1, 2, 8, 8), max_count=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        counts_to_events(torch.zeros(1, 2, 8, 8))


# ------------------------------------------------------------------ C ABI
def test_library_exports_slot_emit():
    from bmc_hip import lib
    assert "bmc_slot_emit" in lib.EXPORTS and lib.has_symbol("bmc_slot_emit")


def test_slot_emit_struct_layout_matches_header():
    import abi_ref
    from bmc_hip import slots
    fields = ["xs", "ys", "ps", "index_in", "index_out", "capacity"]
    structs, constants = abi_ref.compiled_header()
    size, compiled = structs["bmc_slot_emit_t"]
    dt = slots.SLOT_EMIT_DTYPE
    assert [size] + [compiled[f][0] for f in fields] == [dt.itemsize] + [dt.fields[f][1] for f in fields]
    assert [constants["BMC_SLOT_EMIT_MAX_PARTS"], structs["bmc_slot_t"][0], structs["bmc_slot_events_t"][0]] == [
        slots.MAX_EMIT_PARTS, slots.SLOT_DTYPE.itemsize, slots.SLOT_EVENTS_DTYPE.itemsize]
    assert dt.names == tuple(fields) and dt.itemsize == 48


# ------------------------------------------------------------------ ISA and source of csrc/slot_emit.hip
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_emit_kernels_isa(tmp_path):
    """No flat_* accesses, no scratch, no atomics on global memory, no sleep / spin instructions in the two kernels."""
    from test_isa_hygiene import CSRC, _kernels
    o = os.path.join(tmp_path, "slot_emit.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", o, os.path.join(CSRC, "slot_emit.hip")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    ks = {n: k for n, k in _kernels(o).items() if "NumVgprs" in k}
    assert len(ks) == 2 and any("slot_emit_count_kernel" in n for n in ks) and any("slot_emit_write_kernel" in n for n in ks)
    for n, k in ks.items():
        assert k["flat"] == 0 and k["ScratchSize"] == 0 and k["Occupancy"] >= 4, (n, k)
    code = [ln.split(";")[0] for ln in open(o)]
    assert not [ln for ln in code if re.search(r"\b(global_atomic|flat_atomic|buffer_atomic|s_sleep|s_sethalt)", ln)]
    assert [ln for ln in code if "global_store_short" in ln] and [ln for ln in code if "global_store_byte" in ln]
    assert [ln for ln in code if "v_rndne_f32" in ln]                  # rint: round-half-to-even in hardware


def test_emit_source_has_no_wait_on_global_memory():
    """The property 'no backward branch whose body only polls global memory' is awkward to state on the assembly (the compiler
    rotates and unrolls the loops), so it is stated on the source: the file has no `while` / `do` loop, no volatile or atomic
    access, no fence, and every `for` advances its own induction variable by a constant or a power of two -- every loop is
    counted, none re-reads a flag that another workgroup would have to write.  The file is read with the headers that hold what
    it shares with slot_emit_timed.hip (slot_k.h, slot_emit_k.h)."""
    from test_isa_hygiene import CSRC
    src = "".join(open(os.path.join(CSRC, f)).read() for f in ("slot_k.h", "slot_emit_k.h", "slot_emit.hip"))
    body = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(while|do|goto|volatile)\b", body)
    assert not re.search(r"atomic|__threadfence|__builtin_amdgcn_fence|__builtin_amdgcn_s_sleep|asm", body)
    fors = re.findall(r"\bfor \(([^;]*);([^;]*);([^)]*)\)", body)
    assert len(fors) >= 8
    for init, cond, step in fors:
        var = re.match(r"\s*(?:unsigned|int|long long)\s+(\w+)\s*=", init).group(1)
        assert re.fullmatch(r"\s*(\+\+%s|%s \+= \w+|%s >>= 1|%s <<= 1)\s*" % ((var,) * 4), step), (init, cond, step)
        assert re.search(r"\b%s\b" % var, cond)
