"""CPU checks of the timed event output (infer.MultiStreamSR(emit_events=True, event_times="linear"),
csrc/slot_emit_timed.hip): the restatement (event_times_ref.emit_timed_np) against the reference's own clouds, the rank table
against exact fractions, the argument checks, the layout of bmc_slot_emit_timed_t, the exports, and the gfx950 code and the
source of the new kernels."""
import os
import re
import subprocess
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

from event_output_ref import emit_np
from event_times_ref import T0, T1, emit_timed_np, event_jn_np, exact_key_np, times_np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"

# Several float32 roundings at values <= 1 (each <= 6e-8: the reference's linspace works in float32) stay below 1e-6, and 1e-6
# is below half the smallest gap between distinct times, 0.99 / (254 * 253) / 2 = 7.7e-6: derived, not measured.
TOL = 1e-6


# ------------------------------------------------------------------ the definition against the reference
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_restatement_against_the_reference_clouds(k):
    z = np.load(os.path.join(HERE, "golden", "event_times.npz"))
    q, cloud = z["q%d" % k], z["cloud%d" % k]
    sH = q.shape[1]
    xs, ys, ps, ts, q2 = emit_timed_np(q.astype(np.float32))
    assert np.array_equal(q2, q) and len(xs) == len(cloud) == q.sum()
    rx, ry, rt, rp = cloud[:, 0].astype(np.int64), sH - 1 - cloud[:, 1].astype(np.int64), cloud[:, 2], cloud[:, 3].astype(np.int64)
    assert (np.diff(ts) >= 0).all() and (np.diff(rt) >= 0).all()       # both non-decreasing in t
    err = np.abs(rt.astype(np.float64) - ts.astype(np.float64))
    print("image", k, "events", len(ts), "max |t_ref - t|", err.max())
    assert (err <= TOL).all()                                          # position by position
    cuts = np.flatnonzero(np.diff(ts.astype(np.float64)) > TOL) + 1    # runs of positions whose times agree to TOL
    runs = 0
    for a, b in zip(np.r_[0, cuts], np.r_[cuts, len(ts)]):
        mine = sorted(zip(xs[a:b].tolist(), ys[a:b].tolist(), ps[a:b].tolist()))
        assert mine == sorted(zip(rx[a:b].tolist(), ry[a:b].tolist(), rp[a:b].tolist())), (a, b)
        runs += 1
    assert runs == len(np.unique(exact_key_np(*event_jn_np(q))))
    if k < 2:
        assert len(ts) >= 500 and runs >= 10 and {1, 2, 3, 5} <= set(q.ravel().tolist())
    if k == 1:
        assert (q > 30).sum() >= 5


def test_restatement_small_example():
    """[[2, 0], [1, 3]] / [[0, 0], [0, 3]]: times 0.01 (j = 0; four of them, in flat order), 0.505 (two), 1.0 (three)."""
    P = np.array([[[2.0, 0.0], [1.0, 3.0]], [[0.0, 0.0], [0.0, 3.0]]], np.float32)
    xs, ys, ps, ts, q = emit_timed_np(P)
    assert xs.tolist() == [0, 0, 1, 1, 1, 1, 0, 1, 1] and ys.tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 0]
    assert ps.tolist() == [1, 1, 1, -1, 1, -1, 1, 1, -1]
    assert ts.tolist() == [np.float32(0.01)] * 4 + [np.float32(0.01 + 0.99 * 1 / 2)] * 2 + [1.0] * 3 and ts.dtype == np.float32
    plain = emit_np(P)
    assert sorted(zip(xs, ys, ps)) == sorted(zip(*plain[:3]))          # the same events as the untimed stream
    assert (T0, T1) == (0.01, 1.0) and times_np([0], [1])[0] == np.float32(0.01)


def test_time_order_follows_the_exact_key():
    """The rounded float32 time never contradicts the exact order: non-decreasing along increasing keys, for every (j, n)."""
    n, j = np.meshgrid(np.arange(1, 256), np.arange(255), indexing="ij")
    ok = j < n
    n, j = n[ok], j[ok]
    order = np.argsort(exact_key_np(j, n), kind="stable")
    t = times_np(j, n)[order]
    assert (np.diff(t) >= 0).all() and t[0] == np.float32(0.01) and t[-1] == 1.0
    keys = exact_key_np(j, n)[order]
    assert (np.diff(t.astype(np.float64))[np.diff(keys) > 0] > 2 * TOL).all()     # distinct rationals: distinct times, far apart


# ------------------------------------------------------------------ the rank table
def test_rank_table_against_fractions():
    from bmc_hip import slots
    table = slots.emit_rank_table_np()
    assert table.shape == (256, 256) and table.dtype == np.uint16
    frac = lambda n, j: Fraction(j, n - 1) if n > 1 else Fraction(0)
    every = sorted({frac(n, j) for n in range(1, 256) for j in range(n)})
    assert every == sorted({Fraction(p, d) for d in range(1, 255) for p in range(d + 1)}) and len(every) < 1 << 16
    rank = {f: r for r, f in enumerate(every)}
    for n in range(1, 256):
        assert table[n, :n].tolist() == [rank[frac(n, j)] for j in range(n)], n
    assert table[1, 0] == 0 and table[255, 254] == len(every) - 1 and (table[0] == 0).all()
    mask = np.arange(256)[None, :] >= np.arange(256)[:, None]
    assert (table[mask] == 0).all()                                    # entries with j >= n are unused and zero


# ------------------------------------------------------------------ argument checks (no device needed)
def _session(**kw):
    from infer import MultiStreamSR
    return MultiStreamSR(torch.nn.Identity(), 2, n_c=16, scale=4, **kw)


def _frames():
    return torch.zeros(4, 2, 10, 16), torch.zeros(4, 2, 40, 64)


def _event_args():
    cols = lambda n: (torch.ones(n, dtype=torch.int16), torch.ones(n, dtype=torch.int16), torch.ones(n, dtype=torch.float64))
    lr_index = np.stack([20 * np.arange(4), 20 * np.arange(4) + 40], 1)
    gt_index = np.stack([80 * np.arange(4), 80 * np.arange(4) + 160], 1)
    return dict(lr=cols(100), gt=cols(400), lr_index=lr_index, gt_index=gt_index, lr_size=(10, 16), gt_size=(40, 64))


def test_session_event_times_values():
    assert _session().event_times is None and _session(emit_events=True).event_times is None
    assert _session(emit_events=True, event_times="linear").event_times == "linear"
    for bad in ("random", "Linear", True, 1, ""):
        with pytest.raises(ValueError, match="event_times"):
            _session(emit_events=True, event_times=bad)
    with pytest.raises(ValueError, match="emit_events=True"):
        _session(event_times="linear")


def test_timed_session_refuses_max_count_above_255():
    assert _session(emit_events=True, event_times="linear", max_count=255).max_count == 255
    assert _session(emit_events=True, max_count=256).max_count == 256  # untimed: as before
    for bad in (256, 32767):
        with pytest.raises(ValueError, match="max_count <= 255"):
            _session(emit_events=True, event_times="linear", max_count=bad)


@pytest.mark.parametrize("kind", ["open", "open_events"])
def test_window_event_capacity_needs_a_timed_session(kind):
    for ms in (_session(), _session(emit_events=True)):
        with pytest.raises(ValueError, match="event_times='linear'"):
            (ms.open(*_frames(), window_event_capacity=100) if kind == "open"
             else ms.open_events(window_event_capacity=100, **_event_args()))
        assert not ms.sched.pending() and ms._size is None


@pytest.mark.parametrize("kind", ["open", "open_events"])
@pytest.mark.parametrize("bad", [0, -5, 1.5, "many", True, (1 << 28) + 1])
def test_window_event_capacity_must_be_a_positive_integer(kind, bad):
    ms = _session(emit_events=True, event_times="linear")
    with pytest.raises(ValueError, match="window_event_capacity"):
        (ms.open(*_frames(), window_event_capacity=bad) if kind == "open"
         else ms.open_events(window_event_capacity=bad, **_event_args()))
    assert not ms.sched.pending() and ms._size is None
    with pytest.raises(ValueError, match="GPU"):                       # a good one passes the host checks
        ms.open(*_frames(), window_event_capacity=1000)


def test_evaluate_recordings_passes_event_times_through():
    from infer import evaluate_recordings
    with pytest.raises(ValueError, match="event_times"):
        evaluate_recordings(torch.nn.Identity(), [_frames()], 2, n_c=16, emit_events=True, event_times="random")
    with pytest.raises(ValueError, match="max_count <= 255"):
        evaluate_recordings(torch.nn.Identity(), [_frames()], 2, n_c=16, emit_events=True, event_times="linear", max_count=300)
    with pytest.raises(ValueError, match="event_times='linear'"):
        evaluate_recordings(torch.nn.Identity(), [_frames()], 2, n_c=16, emit_events=True, window_event_capacity=10)


def test_slots_emit_timed_refusals():
    from bmc_hip import slots
    pred, parts, scratch = torch.zeros(2, 2, 8, 8), torch.zeros(2, dtype=torch.int32), torch.zeros(8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no timed emit entries"):
        slots.emit_timed(types.SimpleNamespace(S=2, emit=True, timed=False), pred, 255, 1, parts, scratch, 10)
    table = types.SimpleNamespace(S=2, emit=True, timed=True)
    with pytest.raises(ValueError, match="use emit_timed"):
        slots.emit(table, pred, 255, 1, parts)
    for bad in (0, 256, 1.0, True):
        with pytest.raises(ValueError, match="max_count"):
            slots.emit_timed(table, pred, bad, 1, parts, scratch, 10)
    for bad in (0, -1, 2.0, (1 << 28) + 1):
        with pytest.raises(ValueError, match="window_capacity"):
            slots.emit_timed(table, pred, 255, 1, parts, scratch, bad)
    with pytest.raises(ValueError, match="GPU tensor"):
        slots.emit_timed(table, pred, 255, 1, parts, scratch, 10)      # a CPU tensor: there is no CPU path
    with pytest.raises(ValueError, match="timed=True needs emit=True"):
        slots.SlotTable(2, "cpu", timed=True)
    assert slots.EMIT_TIMED_LAUNCHES == 0


def test_scratch_size():
    """8 bytes per event of the window capacity per slot, the slot's total, 256 digit bases and 256 words per histogram row;
    rows = max(nparts, blocks of 4096 records)."""
    from bmc_hip import slots
    assert slots.emit_timed_scratch_bytes(1, 1, 1) == 8 + 8 + 1024 + 1024
    assert slots.emit_timed_scratch_bytes(3, 14, 100000) == 3 * (800000 + 8 + 1024 + 1024 * 25)
    assert slots.emit_timed_scratch_bytes(2, 338, 4096) == 2 * (8 * 4096 + 8 + 1024 + 1024 * 338)
    with pytest.raises(ValueError, match="window_capacity"):
        slots.emit_timed_scratch_bytes(1, 1, 0)


def test_counts_to_events_times_refusals():
    from bmc_hip.encodings import counts_to_events
    with pytest.raises(ValueError, match="times"):
        counts_to_events(torch.zeros(1, 2, 8, 8), times="random")
    with pytest.raises(ValueError, match="max_count <= 255"):
        counts_to_events(torch.zeros(1, 2, 8, 8), max_count=256, times="linear")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        counts_to_events(torch.zeros(1, 2, 8, 8), times="linear")


def test_tool_knows_the_option():
    src = open(os.path.join(ROOT, "tools", "multistream_infer.py")).read()
    assert '"--event-times"' in src and "event_times=" in src


# ------------------------------------------------------------------ C ABI
def test_library_exports_slot_emit_timed():
    from bmc_hip import lib
    for name in ("bmc_slot_emit_timed", "bmc_slot_emit_timed_scratch_bytes"):
        assert name in lib.EXPORTS and lib.has_symbol(name)
    assert lib._slot_emit_timed_ws(0, 1, 1) == -1 and lib._slot_emit_timed_ws(1, 1, (1 << 28) + 1) == -1


def test_slot_emit_timed_struct_layout_matches_header():
    import abi_ref
    from bmc_hip import slots
    fields = ["xs", "ys", "ps", "index_in", "index_out", "capacity", "ts"]
    structs, constants = abi_ref.compiled_header()
    size, compiled = structs["bmc_slot_emit_timed_t"]
    dt = slots.SLOT_EMIT_TIMED_DTYPE
    assert [size] + [compiled[f][0] for f in fields] == [dt.itemsize] + [dt.fields[f][1] for f in fields]
    assert [structs["bmc_slot_emit_t"][0]] + [constants["BMC_SLOT_EMIT_TIMED_" + c] for c in ("MAX_COUNT", "BLOCK", "MAX_WINDOW")] == [
        slots.SLOT_EMIT_DTYPE.itemsize, slots.MAX_COUNT_TIMED, 4096, slots.MAX_WINDOW_CAPACITY]
    assert [constants["BMC_EVENT_T0"], constants["BMC_EVENT_T1"]] == [slots.EVENT_T0, slots.EVENT_T1] == [T0, T1]
    assert dt.names == tuple(fields) and dt.itemsize == 56
    assert dt.names[:6] == slots.SLOT_EMIT_DTYPE.names                 # the fields of bmc_slot_emit_t, then ts
    assert all(dt.fields[f][1] == slots.SLOT_EMIT_DTYPE.fields[f][1] for f in slots.SLOT_EMIT_DTYPE.names)


# ------------------------------------------------------------------ ISA and source of csrc/slot_emit_timed.hip
KERNELS = ("emit_timed_count_kernel", "emit_timed_scan_kernel", "emit_timed_expand_kernel", "emit_timed_hist_kernel",
           "emit_timed_scatter_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_timed_emit_kernels_isa(tmp_path):
    """No flat_* accesses, no scratch memory, no atomics on global memory, no sleep / halt; 256-thread workgroups of at most
    64 VGPRs and under 10 KB of LDS: occupancy 8 waves per SIMD, asserted.  The histograms use LDS atomics (ds_add), the
    columns leave through vector stores of their own widths, the time is computed in float64."""
    from test_isa_hygiene import CSRC, _kernels
    o = os.path.join(tmp_path, "slot_emit_timed.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", o, os.path.join(CSRC, "slot_emit_timed.hip")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    ks = {n: k for n, k in _kernels(o).items() if "NumVgprs" in k}
    assert len(ks) == len(KERNELS) and all(any(want in n for n in ks) for want in KERNELS)
    for n, k in ks.items():
        assert k["flat"] == 0 and k["ScratchSize"] == 0 and k["Occupancy"] == 8 and k["NumVgprs"] <= 64, (n, k)
    code = [ln.split(";")[0] for ln in open(o)]
    assert not [ln for ln in code if re.search(r"\b(global_atomic|flat_atomic|buffer_atomic|s_sleep|s_sethalt|scratch_)", ln)]
    assert [ln for ln in code if "ds_add_u32" in ln]
    for store in ("global_store_short", "global_store_byte", "global_store_dword ", "global_store_dwordx2"):
        assert [ln for ln in code if store in ln.replace("\t", " ")], store
    assert [ln for ln in code if "v_rndne_f32" in ln] and [ln for ln in code if "v_cvt_f32_f64" in ln]
    assert [ln for ln in code if "v_div_scale_f64" in ln]              # an IEEE float64 division, not a reciprocal
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", open(o).read())]
    assert len(lds) == len(KERNELS) and max(lds) <= 10240


def test_timed_emit_source_has_no_wait_and_six_launches():
    """As test_event_output_cpu states it for slot_emit.hip: no `while` / `do` loop, no volatile access, no fence, no inline
    assembly, every `for` advances its own induction variable -- every loop is counted, none polls a flag.  The only atomics are
    the two LDS histogram increments.  One call launches six kernels (slots.EMIT_TIMED_KERNELS).  The file is read with the
    headers that hold what it shares with slot_emit.hip (slot_k.h, slot_emit_k.h)."""
    from bmc_hip import slots
    from test_isa_hygiene import CSRC
    src = "".join(open(os.path.join(CSRC, f)).read() for f in ("slot_k.h", "slot_emit_k.h", "slot_emit_timed.hip"))
    body = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(while|do|goto|volatile)\b", body)
    assert not re.search(r"__threadfence|__builtin_amdgcn_fence|__builtin_amdgcn_s_sleep|asm", body)
    atomics = re.findall(r"\w*[aA]tomic\w*\([^;]*;", body)
    assert len(atomics) == 2 and all(a.startswith("atomicAdd(&lh[") for a in atomics) and "__shared__ unsigned lh[256]" in body
    fors = re.findall(r"\bfor \(([^;]*);([^;]*);([^)]*)\)", body)
    assert len(fors) >= 15
    for init, cond, step in fors:
        var = re.match(r"\s*(?:unsigned|int|long long)\s+(\w+)\s*=", init).group(1)
        assert re.fullmatch(r"\s*(\+\+%s|%s \+= \w+|%s >>= 1|%s <<= 1)\s*" % ((var,) * 4), step), (init, cond, step)
        assert re.search(r"\b%s\b" % var, cond)
    assert len(re.findall(r"hipLaunchKernelGGL\(", body)) == slots.EMIT_TIMED_KERNELS == 6
    assert open(os.path.join(CSRC, "Makefile")).read().count("slot_emit_timed.hip") == 1
