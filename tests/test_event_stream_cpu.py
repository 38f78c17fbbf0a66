"""CPU checks of the continuous event stream (infer.MultiStreamSR(continuous=True); csrc/slot_emit_trimmed.hip,
bmc_slot_emit_trimmed; include/bmc_hip_stream.h): the bisection for k(n) against the brute-force count, the prefix property the
trim rests on, a cut on a run of ties, the concatenation of half-overlapping windows, the table layout, every host refusal, the
companion header against the library's ABI text and the binding, and the compiler's figures for the two new kernels.  Every
comparison is exact."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

import abi_ref
from event_clock_ref import SPANS, emit_clocked_np
from event_stream_ref import (cuts_np, emit_trimmed_np, half_overlapping_spans, kept_bisect_np, kept_brute_np, time_np)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bmcnet-esr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def _cuts_of(span):
    """The cuts the bisection is checked at: below t_first, t_first itself, the time of rational 1/2, t_last, the next float64
    above it, +inf."""
    t_first, t_last = np.float64(span[0]), np.float64(span[1])
    return [t_first - 1.0, t_first, time_np(1, 3, span), t_last, np.nextafter(t_last, np.inf), np.inf]


# ------------------------------------------------------------------ 1. k(n)
@pytest.mark.parametrize("span", SPANS)
def test_bisection_equals_the_brute_force_count(span):
    for t_cut in _cuts_of(span):
        got = [kept_bisect_np(n, span, t_cut) for n in range(256)]
        assert got == [kept_brute_np(n, span, t_cut) for n in range(256)], t_cut
    below, at_first, half, at_last, above, inf = ([kept_brute_np(n, span, c) for n in range(256)] for c in _cuts_of(span))
    assert below == at_first == [0] * 256                               # the earliest time of a window is t_first + 0.01 dt
    assert above == inf == list(range(256))                             # t_last itself is the latest
    if span[1] > span[0]:
        assert at_last[1] == 1 and at_last[2:] == list(range(1, 255))   # j = n - 1 lands on t_last exactly: cut, strictly
        assert half[3] == 1 and half[5] == 2 and half[2] == 1           # 1/2 and 2/4 are on the cut: dropped
    else:
        assert at_last == [0] * 256                                     # a degenerate span: all dropped at t_first ...
        assert [kept_brute_np(n, span, np.nextafter(span[0], np.inf)) for n in range(256)] == list(range(256))      # ... or all kept


def test_time_is_non_decreasing_in_j_for_every_n():
    """What the bisection rests on."""
    for span in SPANS:
        for n in range(2, 256):
            assert (np.diff(time_np(np.arange(n), np.full(n, n), span)) >= 0).all()


# ------------------------------------------------------------------ 2. the kept set
def _random_P(rng, sH=5, sW=7):
    P = rng.integers(0, 9, (2, sH, sW)).astype(np.float32)
    P[0, 0, 0], P[1, -1, -1] = 255.0, 254.0
    return P


def test_kept_set_is_a_prefix_for_random_cuts():
    rng = np.random.default_rng(3)
    for span in SPANS[1:]:
        for _ in range(6):
            P = _random_P(rng)
            t_cut = np.float64(span[0]) + rng.uniform(-0.1, 1.1) * (np.float64(span[1]) - np.float64(span[0]))
            xs, ys, ps, ts, dropped = emit_trimmed_np(P, span, t_cut)               # (asserts the prefix)
            full = emit_clocked_np(P, span)
            k = len(xs)
            assert k + dropped == len(full[0]) and all(a.tobytes() == b[:k].tobytes() for a, b in zip((xs, ys, ps, ts), full))
            q = full[4].ravel()
            assert k == sum(kept_brute_np(int(n), span, t_cut) for n in q)          # per element: its first k(n) events


def test_a_cut_on_a_tie_run_drops_the_whole_run():
    P = np.zeros((2, 2, 3), np.float32)
    P[0, 0, 0], P[0, 1, 1], P[1, 0, 2], P[1, 1, 0] = 3.0, 5.0, 2.0, 3.0       # rationals 0, 1/2 (x3: 1/2, 2/4, 1/2), 1/4, 3/4, 1
    span = SPANS[2]
    t_half = time_np(1, 3, span)
    assert t_half == time_np(2, 5, span)                                # equal rationals: one time
    full = emit_clocked_np(P, span)[3]
    assert (full == t_half).sum() == 3
    ts = emit_trimmed_np(P, span, t_half)[3]
    assert len(ts) == (full < t_half).sum() == 5 and (ts < t_half).all()   # j = 0 of each of the four elements, and 1/4
    assert len(emit_trimmed_np(P, span, np.nextafter(t_half, np.inf))[3]) == 8      # just above: the run is kept whole


def test_three_half_overlapping_windows_concatenate_in_time_order():
    rng = np.random.default_rng(5)
    spans = half_overlapping_spans(5, 123456789.0, 1524.0)              # windows 0 .. 2 predict items 1 .. 3
    cuts = cuts_np(spans, 3)
    assert cuts.tolist() == [spans[2, 0], spans[3, 0], np.inf]
    Ps = [_random_P(rng) for _ in range(3)]
    trimmed = np.concatenate([emit_trimmed_np(P, spans[i + 1], cuts[i])[3] for i, P in enumerate(Ps)])
    plain = np.concatenate([emit_clocked_np(P, spans[i + 1])[3] for i, P in enumerate(Ps)])
    assert (np.diff(trimmed) >= 0).all() and not (np.diff(plain) >= 0).all() and 0 < len(trimmed) < len(plain)
    assert trimmed[0] >= spans[1, 0] and trimmed[-1] == spans[3, 1]
    apart = np.stack([spans[:, 0], spans[:, 0] + 1523.0], 1)            # spans that do not overlap: nothing is dropped
    assert all(emit_trimmed_np(P, apart[i + 1], cuts_np(apart, 3)[i])[4] == 0 for i, P in enumerate(Ps))


def test_the_sessions_cuts_are_the_restated_ones():
    from infer_parts import EventStream
    for L, n in ((5, 3), (4, 2), (3, 1), (6, 2), (4, 3)):               # (seqn = 3: n = L - 2; also shorter and longer tables)
        spans = half_overlapping_spans(L, 5.0e5, 0.25)
        assert EventStream.cuts(spans, n).tobytes() == cuts_np(spans, n).tobytes(), (L, n)


# ------------------------------------------------------------------ 3. the table
def test_table_layout_gains_only_a_trailing_section():
    from bmc_hip import slots
    assert slots.SLOT_TRIM_DTYPE.itemsize == 16 and slots.SLOT_TRIM_DTYPE.names == ("t_cut", "dropped")
    for S in (1, 3, 5):
        for kw in (dict(emit=True, timed=True, clock=True), dict(events=True, hot=True, emit=True, timed=True, clock=True),
                   dict(events=True, hot=True, emit=True, timed=True, clock=True, render=5, voxel=True, quality=True)):
            base = slots.table_layout(S, **kw)
            assert slots.table_layout(S, trim=False, **kw) == base
            sections, nbytes = slots.table_layout(S, trim=True, **kw)
            assert sections[:-1] == base[0] and sections[-1] == ("trim", slots.SLOT_TRIM_DTYPE, base[1])
            assert nbytes == base[1] + 16 * S and base[1] % 8 == 0
        for kw in ({}, dict(events=True), dict(emit=True), dict(emit=True, timed=True), dict(events=True, hot=True, render=2),
                   dict(voxel=True, quality=True)):
            assert slots.table_layout(S, trim=False, **kw) == slots.table_layout(S, **kw)
            with pytest.raises(ValueError, match="trim=True needs clock=True"):
                slots.table_layout(S, trim=True, **kw)
    sections, total = slots.table_layout(3, events=True, emit=True, timed=True, clock=True, hot=True)      # today's literals
    assert [off for _, _, off in sections] == [0, 120, 696, 864, 936] and total == 1128
    with pytest.raises(ValueError, match="trim=True needs clock=True"):
        slots.SlotTable(2, "cpu", emit=True, timed=True, trim=True)


def test_slots_emit_trimmed_refusals():
    from bmc_hip import slots, stream_lib
    pred, parts, scratch = torch.zeros(2, 2, 8, 8), torch.zeros(4, dtype=torch.int32), torch.zeros(8, dtype=torch.uint8)
    for t in (types.SimpleNamespace(S=2, emit=True, timed=True, clock=True), types.SimpleNamespace(S=2, emit=True, timed=True, clock=True, trim=False),
              types.SimpleNamespace(S=2, emit=True, timed=True, clock=False, trim=True)):
        with pytest.raises(ValueError, match="no trim entries"):
            slots.emit_trimmed(t, pred, 255, 1, parts, scratch, 10)
    table = types.SimpleNamespace(S=2, emit=True, timed=True, clock=True, trim=True)
    for bad in (0, 256, 1.0, True):
        with pytest.raises(ValueError, match="max_count"):
            slots.emit_trimmed(table, pred, bad, 1, parts, scratch, 10)
    for bad in (0, -1, 2.0, (1 << 28) + 1):
        with pytest.raises(ValueError, match="window_capacity"):
            slots.emit_trimmed(table, pred, 255, 1, parts, scratch, bad)
    with pytest.raises(ValueError, match="GPU tensor"):
        slots.emit_trimmed(table, pred, 255, 1, parts, scratch, 10)
    assert stream_lib.TRIM_PARTS == 2 and slots.EMIT_TIMED_KERNELS == 6


# ------------------------------------------------------------------ 4. the host refusals
def _session(**kw):
    from infer import MultiStreamSR
    return MultiStreamSR(torch.nn.Identity(), 2, n_c=16, scale=4, **kw)


def _continuous():
    return _session(emit_events=True, event_times="linear", continuous=True)


def _event_args():
    cols = lambda n: (torch.ones(n, dtype=torch.int16), torch.ones(n, dtype=torch.int16), torch.ones(n, dtype=torch.float64))
    return dict(lr=cols(100), lr_index=np.stack([20 * np.arange(4), 20 * np.arange(4) + 40], 1), lr_size=(10, 16))


def test_continuous_needs_linear_event_times():
    for kw in ({}, dict(emit_events=True), dict(keep_predictions=True)):
        with pytest.raises(ValueError, match="continuous=True needs event_times='linear'"):
            _session(continuous=True, **kw)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="continuous must be True or False"):
            _session(emit_events=True, event_times="linear", continuous=bad)
    assert _continuous().continuous is True and _session().continuous is False
    assert _session(emit_events=True, event_times="linear").continuous is False


def test_a_continuous_session_needs_the_clock_of_every_recording():
    for kind in ("open", "open_events"):
        ms = _continuous()
        with pytest.raises(ValueError, match="no clock to cut on"):
            ms.open(torch.zeros(4, 2, 10, 16)) if kind == "open" else ms.open_events(**_event_args())
        assert not ms.sched.pending() and ms._size is None and not ms._recs


@pytest.mark.parametrize("bad,match", [
    (np.array([[0.0, 2.0], [3.0, 5.0], [2.0, 4.0], [4.0, 6.0]]), "t_first does not decrease"),
    (np.array([[0.0, 2.0], [1.0, 3.0], [2.0, 4.0], [3.0, np.inf]]), "finite"),
    (np.array([[0.0, 2.0], [np.nan, 3.0], [2.0, 4.0], [3.0, 5.0]]), "finite"),
    (np.array([[0.0, 2.0], [1.0, 3.0], [-np.inf, 4.0], [3.0, 5.0]]), "finite"),
])
def test_bad_spans_are_refused_and_leave_no_trace(bad, match):
    for kind in ("open", "open_events"):
        ms = _continuous()
        with pytest.raises(ValueError, match=match):
            ms.open(torch.zeros(4, 2, 10, 16), spans=bad) if kind == "open" else ms.open_events(spans=bad, **_event_args())
        assert not ms.sched.pending() and ms._size is None and not ms._recs


def test_good_spans_pass_the_host_checks():
    """Items the windows do not predict may lie anywhere (item 0; with seqn = 3 and L = 4 the windows predict items 1 and 2), and
    a session without the option takes spans that run backwards, as before."""
    good = np.array([[9.0, 9.5], [1.0, 3.0], [2.0, 4.0], [0.0, 0.5]])
    for ms in (_continuous(), _session(emit_events=True, event_times="linear")):
        with pytest.raises(ValueError, match="GPU"):
            ms.open(torch.zeros(4, 2, 10, 16), spans=good)
    with pytest.raises(ValueError, match="GPU"):
        _session(emit_events=True, event_times="linear").open(torch.zeros(4, 2, 10, 16), spans=good[::-1].copy())
    with pytest.raises(ValueError, match="GPU"):
        _continuous().open_events(lr_ts=np.arange(100.0), **_event_args())


def test_counts_to_events_cut_refusals():
    from bmc_hip.encodings import counts_to_events
    P = torch.zeros(2, 2, 8, 8)
    with pytest.raises(ValueError, match="cuts needs spans"):
        counts_to_events(P, times="linear", cuts=[1.0, 2.0])
    for bad in ([1.0], [[1.0, 2.0]], ["a", "b"]):
        with pytest.raises(ValueError, match="one number per image"):
            counts_to_events(P, times="linear", spans=[[0.0, 1.0]] * 2, cuts=bad)
    with pytest.raises(ValueError, match="NaN"):
        counts_to_events(P, times="linear", spans=[[0.0, 1.0]] * 2, cuts=[np.nan, 1.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        counts_to_events(P, times="linear", spans=[[0.0, 1.0]] * 2, cuts=[np.inf, 0.5])


def test_evaluate_recordings_and_the_tool_take_the_option():
    import inspect
    import infer
    assert inspect.signature(infer.evaluate_recordings).parameters["continuous"].default is False
    assert inspect.signature(infer.MultiStreamSR.__init__).parameters["continuous"].default is False
    with pytest.raises(ValueError, match="continuous=True needs event_times='linear'"):
        infer.evaluate_recordings(torch.nn.Identity(), {}, 2, continuous=True)
    assert '"--continuous"' in open(os.path.join(ROOT, "tools", "multistream_infer.py")).read()


# ------------------------------------------------------------------ 5. header, ABI text, binding, exports, build
def test_companion_header_matches_its_abi_text_and_binding():
    from bmc_hip import lib, slots, stream_lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(abi_ref.INCLUDE, "bmc_hip_stream.h")).read(), flags=re.S)
    declared = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?[a-z][a-z ]*\*?)\s*\b(bmc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, re.M):
        params = [p.strip() for p in params.split(",")]
        declared[name] = [abi_ref.classify(ret)] + ([] if params == ["void"] else [abi_ref.classify(p) for p in params])
    assert sorted(declared) == sorted(stream_lib.FUNCTIONS) == ["bmc_slot_emit_trimmed", "bmc_stream_abi"]
    assert not set(declared) & set(lib.FUNCTIONS) and set(lib.EXPORTS) == set(abi_ref.functions())      # bmc_hip.h does not grow
    want = ["i4", "p", "p", "p", "p", "i4", "p", "i4", "i4", "i4", "i4", "p", "p", "p", "i8", "p"]
    assert [c.split(":")[0] for c in stream_lib.FUNCTIONS["bmc_slot_emit_trimmed"]] == want == declared["bmc_slot_emit_trimmed"]
    clocked = [c.split(":")[0] for c in lib.FUNCTIONS["bmc_slot_emit_clocked"]]
    assert want == clocked[:4] + ["p"] + clocked[4:]                    # the clocked call's arguments and a fifth table
    assert stream_lib.FUNCTIONS["bmc_slot_emit_trimmed"][4] == "p:bmc_slot_trim_t"
    assert stream_lib._slot_emit_trimmed.restype is C.c_int and len(stream_lib._slot_emit_trimmed.argtypes) == 15
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    body = ['printf("size %zu\\n", sizeof(bmc_slot_trim_t));', 'printf("align %zu\\n", _Alignof(bmc_slot_trim_t));',
            'printf("t_cut %zu\\n", offsetof(bmc_slot_trim_t, t_cut));', 'printf("dropped %zu\\n", offsetof(bmc_slot_trim_t, dropped));',
            'printf("BMC_SLOT_TRIM_PARTS %d\\n", BMC_SLOT_TRIM_PARTS);']
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "bmc_hip_stream.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(body)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run([cc, "-I" + abi_ref.INCLUDE, os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    compiled = dict(zip(out[::2], map(int, out[1::2])))
    st = stream_lib.STRUCTS["bmc_slot_trim_t"]
    assert compiled == {"size": st.size, "align": st.align, "t_cut": st.fields["t_cut"].offset, "dropped": st.fields["dropped"].offset,
                        "BMC_SLOT_TRIM_PARTS": stream_lib.TRIM_PARTS} and st.size == slots.SLOT_TRIM_DTYPE.itemsize == 16
    dt = slots.SLOT_TRIM_DTYPE
    assert dt.fields["t_cut"] == (np.dtype("<f8"), 0) and dt.fields["dropped"] == (np.dtype("<u8"), 8)
    assert "bmc_hip_stream.h" not in open(os.path.join(abi_ref.INCLUDE, "bmc_hip.h")).read()


def test_library_exports_and_refusals_before_any_launch():
    from bmc_hip import lib, stream_lib
    for name in ("bmc_slot_emit_trimmed", "bmc_stream_abi"):
        assert lib.has_symbol(name) and name not in lib.EXPORTS
    fn = stream_lib._slot_emit_trimmed
    good = dict(table=64, emit=64, clock=64, trim=64, S=1, pred=64, sH=8, sW=8, mc=255, nparts=1, parts=64, rank=64, scratch=64,
                wcap=10, s=None)                                        # (every check comes before anything touches a device)
    for kw, msg in ((dict(trim=None), b"trim table"), (dict(trim=68), b"trim table"), (dict(clock=None), b"clock table"),
                    (dict(clock=68), b"clock table"), (dict(mc=256), b"max_count"), (dict(mc=0), b"max_count"),
                    (dict(wcap=0), b"window_capacity"), (dict(wcap=(1 << 28) + 1), b"window_capacity"), (dict(scratch=68), b"aligned"),
                    (dict(scratch=None), b"bad arguments"), (dict(S=0), b"bad arguments"), (dict(sH=32768), b"32767"),
                    (dict(nparts=1025), b"nparts"), (dict(table=None), b"bad arguments")):
        assert fn(*{**good, **kw}.values()) == -1, kw
        err = lib.bmc_last_error()
        assert b"bmc_slot_emit_trimmed" in err and msg in err, (kw, err)


def test_makefile_names_the_source_once_and_the_header_as_a_dependency():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert srcs.count("slot_emit_trimmed.hip") == 1 and mk.count("slot_emit_trimmed.hip") == 1 and len(srcs) == len(set(srcs))
    assert mk.count("../../include/bmc_hip_stream.h") == 1
    assert open(os.path.join(CSRC, "abi.hip")).read().count('#include "bmc_hip_stream.h"') == 1


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_trimmed_emit_kernels_isa(tmp_path):
    """The two new kernels: no flat_* accesses, no scratch memory, no atomics on global memory, no sleep / halt; 256-thread
    workgroups of at most 64 VGPRs and under 11 KB of LDS (the expand kernel's 9.3 KB and the tile's q, the keep table and the
    words of the dropped sum): occupancy 8 waves per SIMD, asserted.  The time under the bisection is an IEEE float64 division."""
    from test_isa_hygiene import _kernels
    o = os.path.join(tmp_path, "slot_emit_trimmed.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", o, os.path.join(CSRC, "slot_emit_trimmed.hip")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    ks = {n: k for n, k in _kernels(o).items() if "NumVgprs" in k}
    assert len(ks) == 2 and all(any(want in n for n in ks) for want in ("emit_trimmed_count_kernel", "emit_trimmed_expand_kernel"))
    for n, k in ks.items():
        assert k["flat"] == 0 and k["ScratchSize"] == 0 and k["Occupancy"] == 8 and k["NumVgprs"] <= 64, (n, k)
    code = [ln.split(";")[0] for ln in open(o)]
    assert not [ln for ln in code if re.search(r"\b(global_atomic|flat_atomic|buffer_atomic|s_sleep|s_sethalt|scratch_)", ln)]
    assert [ln for ln in code if "ds_add_u32" in ln] and [ln for ln in code if "v_div_scale_f64" in ln]
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", open(o).read())]
    assert len(lds) == 2 and max(lds) <= 11264


def test_trimmed_emit_source_has_no_wait_and_shares_the_high_pass():
    """As test_event_times_cpu states it for slot_emit_timed.hip: no `while` / `do` loop, no volatile access, no fence, no inline
    assembly, every `for` advances its own induction variable.  The only atomic is the LDS histogram increment.  The file launches
    two kernels of its own; the other four launches are slot_emit_timed.hip's, through the functions slot_emit_k.h declares; the
    time under the bisection is slot_emit_k.h's clock_time, which slot_emit_timed.hip's scatter kernel stores."""
    from bmc_hip import slots
    src = open(os.path.join(CSRC, "slot_emit_trimmed.hip")).read()
    body = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(while|do|goto|volatile)\b", body)
    assert not re.search(r"__threadfence|__builtin_amdgcn_fence|__builtin_amdgcn_s_sleep|asm", body)
    atomics = re.findall(r"\w*[aA]tomic\w*\([^;]*;", body)
    assert len(atomics) == 1 and atomics[0].startswith("atomicAdd(&lh[") and "__shared__ unsigned lh[256]" in body
    for init, cond, step in re.findall(r"\bfor \(([^;]*);([^;]*);([^)]*)\)", body):
        var = re.match(r"\s*(?:unsigned|int|long long)\s+(\w+)\s*=", init).group(1)
        assert re.fullmatch(r"\s*(\+\+%s|%s \+= \w+|%s >>= 1|%s <<= 1)\s*" % ((var,) * 4), step), (init, cond, step)
        assert re.search(r"\b%s\b" % var, cond)
    timed = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "slot_emit_timed.hip")).read())
    header = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "slot_emit_k.h")).read())
    assert len(re.findall(r"hipLaunchKernelGGL\(", body)) == 2 and len(re.findall(r"hipLaunchKernelGGL\(", timed)) == slots.EMIT_TIMED_KERNELS
    assert body.count("bmc_emit_timed_scan_parts(p)") == 1 and body.count("bmc_emit_timed_high_pass(p)") == 1
    assert len(re.findall(r"\bdouble clock_time\(", header)) == 1 and "clock_time(" not in re.sub(r"clock_time\(t_first, dt, j, nq\)", "", timed)
    assert "clock_time(t_first, dt, mid, n)" in body and "clock_time(t_first, dt, j, nq)" in timed
