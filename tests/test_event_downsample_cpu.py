"""The integrate-and-fire event downsampler without a GPU: the two restatements of tests/event_downsample_ref.py against each
other and against hand-written expectations, the conservation law of the accumulators, the capacity, the corollaries, the Python
refusals, the companion header include/bmc_hip_downsample.h against the library's ABI text, a C compile and the binding, the
exports, and the compiler's figures for csrc/event_downsample.hip (LDS bytes, no scratch)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import abi_ref
import event_denoise_ref as N
import event_downsample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _both(cols, H, W, s, T):
    a, b = R.downsample_seq(*cols, H, W, s, T), R.downsample_grouped(*cols, H, W, s, T)
    assert R.same(a, b)
    assert [c.dtype for c in a[:4]] == [np.int16, np.int16, np.float64, np.float64]
    return a


def _law(cols, out, H, W, s, T):
    """Per LR pixel: T * (fires+ - fires-) + a_final == the sum of the steps, |a_final| < T; count <= n // T."""
    xs, ys, _, ps = cols
    h, w = R.lr_size(H, W, s)
    ok = R.counted(xs, ys, ps, H, W)
    steps = np.zeros((h, w), np.int64)
    np.add.at(steps, (ys[ok].astype(np.int64) // s, xs[ok].astype(np.int64) // s), np.where(ps[ok] > 0, 1, -1))
    net = np.zeros((h, w), np.int64)
    np.add.at(net, (out[1].astype(np.int64), out[0].astype(np.int64)), out[3].astype(np.int64))
    assert np.array_equal(T * net + out[4], steps) and (np.abs(out[4]) < T).all()
    assert len(out[0]) <= len(xs) // T
    assert set(np.unique(out[3]).tolist()) <= {-1.0, 1.0}


# ------------------------------------------------------------------ 1. the two restatements, the law, the capacity
@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("H,W,n", [(5, 7, 600), (37, 53, 6000), (64, 96, 20000)])
def test_sequential_and_grouped_forms_agree_and_conserve_steps(H, W, n, s):
    for cols in (N.stream(H, W, n, 0.3, seed=H * W + n + s), R.stream(H, W, n, s, seed=H * W + n + s)):
        for T in (1, max(2, s * s // 2), s * s):
            out = _both(cols, H, W, s, T)
            _law(cols, out, H, W, s, T)
            assert len(out[0]) > 0
    assert len(out[0]) > n // (4 * s * s) and {-1.0, 1.0} == set(out[3].tolist())     # the coherent stream fires often, both ways
    assert np.isnan(cols[3]).any() and (cols[3] == 0).any() and np.signbit(cols[3][cols[3] == 0]).any()
    xs, ys = cols[0].astype(np.int64), cols[1].astype(np.int64)
    assert n < 6000 or ((xs < 0) | (xs >= W) | (ys < 0) | (ys >= H)).any()       # out-of-range events are in the stream


def test_capacity_is_reached_exactly_by_like_signed_events_on_one_pixel():
    for T, k, sign in ((1, 7, 1.0), (4, 5, -1.0), (16, 3, 1.0), (32767, 1, -1.0)):
        cols = R.columns([5] * (k * T), [2] * (k * T), [sign] * (k * T))
        out = _both(cols, 8, 12, 4, T)
        assert len(out[0]) == k == len(cols[0]) // T and (out[3] == sign).all() and (out[0] == 1).all() and (out[1] == 0).all()
        assert np.array_equal(out[2], cols[2][T - 1::T]) and not out[4].any()
        one_short = tuple(c[:-1] for c in cols)
        assert len(_both(one_short, 8, 12, 4, T)[0]) == k - 1 == len(one_short[0]) // T


# ------------------------------------------------------------------ 2. corollaries
def test_corollaries_of_threshold_one():
    H, W, n = 37, 53, 6000
    xs, ys, ts, ps = N.stream(H, W, n, 0.3, seed=3)
    ps = ps * np.random.default_rng(0).integers(1, 4, n)                 # any non-zero weight counts as its sign
    ok = R.counted(xs, ys, ps, H, W)
    out = _both((xs, ys, ts, ps), H, W, 1, 1)                            # s = 1, T = 1: the counted events themselves
    assert R.same(out[:4], (xs[ok], ys[ok], ts[ok], np.sign(ps[ok])))
    for s in (2, 3, 4):                                                  # T = 1: the counted stream, coordinates divided
        out = _both((xs, ys, ts, ps), H, W, s, 1)
        assert R.same(out[:4], ((xs[ok] // s).astype(np.int16), (ys[ok] // s).astype(np.int16), ts[ok], np.sign(ps[ok])))
        assert out[0].max() == (W - 1) // s and out[1].max() == (H - 1) // s


# ------------------------------------------------------------------ 3. hysteresis, ignored events, ties
@pytest.mark.parametrize("T", [2, 3, 16])
def test_hysteresis(T):
    H, W, s = 8, 12, 4
    assert len(_both(R.columns(*R.hysteresis_no_fire(T, 5, 6)), H, W, s, T)[0]) == 0
    cols = R.columns(*R.exact_fire(T, 5, 6))
    out = _both(cols, H, W, s, T)
    assert out[0].tolist() == [1] and out[1].tolist() == [1] and out[3].tolist() == [1.0] and out[2][0] == cols[2][T - 1]
    assert out[4][1, 1] == T - 1                                          # the reset: T-1 further ups do not fire again
    out = _both(R.columns(*R.exact_fire(T, 5, 6, -1.0)), H, W, s, T)
    assert out[3].tolist() == [-1.0] and out[4][1, 1] == -(T - 1)
    assert len(_both(R.columns(*R.alternating(501, 5, 6)), H, W, s, T)[0]) == 0
    xs, ys, ps = R.alternating(8, 5, 6)                                   # ... and with T = 1 every one of them fires
    assert _both(R.columns(xs, ys, ps), H, W, s, 1)[3].tolist() == ps
    # the block adds its pixels: T ups spread over the block's s*s pixels fire once, on the last
    xs, ys = [4 + i % 4 for i in range(T)], [4 + (i // 4) % 4 for i in range(T)]
    out = _both(R.columns(xs, ys, [1.0] * T), H, W, s, T)
    assert len(out[0]) == 1 and out[2][0] == (T - 1) * 1e-6
    # ... and T ups over two LR pixels do not (T >= 2)
    assert len(_both(R.columns([3] * (T - 1) + [4], [0] * T, [1.0] * T), H, W, s, T)[0]) == 0


def test_ignored_events_change_nothing():
    H, W, s, T = 5, 7, 2, 3
    base = R.columns([2, 3, 2, 3, 2, 2, 3, 3], [0, 1, 1, 0, 0, 1, 1, 0], [1.0, 1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0])
    want = _both(base, H, W, s, T)
    assert want[2].tolist() == [2e-6, 7e-6]                               # fires at events 2 and 7: 0, -1, 0, 1, 2, 3 after the reset
    junk = [(2, 0, 0.0), (2, 0, -0.0), (3, 1, float("nan")), (-1, 0, 1.0), (W, 0, 1.0), (2, -1, 1.0), (2, H, -1.0), (7, 4, 1.0),
            (-32768, 32767, 1.0)]
    for at in range(len(base[0]) + 1):
        for x, y, p in junk:
            cols = (np.insert(base[0], at, x), np.insert(base[1], at, y), np.insert(base[2], at, 0.5), np.insert(base[3], at, p))
            got = _both(cols, H, W, s, T)
            assert R.same(got, want), (at, x, y, p)
    edge = _both(R.columns([6] * 3, [4] * 3, [1.0] * 3), H, W, s, T)      # the ragged edge block keeps the same T
    assert edge[0].tolist() == [3] and edge[1].tolist() == [2]


def test_equal_timestamps_act_in_column_order():
    H, W, s, T = 4, 4, 2, 2
    ts = [0.5] * 4
    a = _both(R.columns([0, 1, 0, 1], [0, 0, 1, 1], [1.0, 1.0, -1.0, -1.0], ts), H, W, s, T)      # up up | down down: two fires
    assert a[3].tolist() == [1.0, -1.0] and a[2].tolist() == [0.5, 0.5]
    b = _both(R.columns([0, 0, 1, 1], [0, 1, 0, 1], [1.0, -1.0, 1.0, -1.0], ts), H, W, s, T)      # the same events, interleaved: none
    assert len(b[0]) == 0
    # the result is a function of column order only: shuffled timestamps change the ts column and nothing else
    cols = N.stream(37, 53, 3000, 0.3, seed=9)
    rev = (cols[0], cols[1], cols[2][::-1].copy(), cols[3])
    x, y = _both(cols, 37, 53, 4, 4), R.downsample_seq(*rev, 37, 53, 4, 4)
    assert R.same((x[0], x[1], x[3], x[4]), (y[0], y[1], y[3], y[4])) and len(x[0]) > 0


# ------------------------------------------------------------------ 4. Python refusals
def test_python_refusals():
    from bmc_hip import downsample_lib
    from bmc_hip.encodings import downsample_events, downsample_geometry
    xs, ts = torch.zeros(10, dtype=torch.int16), torch.arange(10, dtype=torch.float64)
    ps = torch.ones(10, dtype=torch.float64)
    for args, match in (((xs, xs, ts, ps, (8, 12), 4), "GPU tensors on one device"),
                        ((xs.int(), xs, ts, ps, (8, 12), 4), "xs must be"), ((xs, xs.int(), ts, ps, (8, 12), 4), "ys must be"),
                        ((xs, xs, ts.float(), ps, (8, 12), 4), "ts must be"), ((xs, xs, ts, ps.float(), (8, 12), 4), "ps must be"),
                        ((xs, xs, ts, None, (8, 12), 4), "ps must be"), ((xs, xs, ts[:9], ps, (8, 12), 4), "ts has 9 entries, xs 10"),
                        ((xs, xs, ts, ps.view(2, 5), (8, 12), 4), "ps must be"), ((xs.numpy(), xs, ts, ps, (8, 12), 4), "xs must be")):
        with pytest.raises(ValueError, match="^downsample_events: .*" + match):
            downsample_events(*args)
    for size, scale, T, match in ((7, 4, None, r"sensor_size = \(H, W\)"), ((0, 12), 4, None, "must be positive"),
                                  ((8, -1), 4, None, "must be positive"), ((8, 12), 0, None, "scale must be"),
                                  ((8, 12), downsample_lib.MAX_SCALE + 1, None, "scale must be"), ((8, 12), 2.0, None, "scale must be"),
                                  ((8, 12), True, None, "scale must be"), ((8, 12), 4, 0, "threshold must be"),
                                  ((8, 12), 4, downsample_lib.MAX_THRESHOLD + 1, "threshold must be"),
                                  ((8, 12), 4, 16.0, "threshold must be"), ((8, 12), 4, True, "threshold must be"),
                                  ((1 << 16, 1 << 16), 1, None, "not below 2\\^31 - 1")):
        with pytest.raises(ValueError, match="^downsample_events: .*" + match):
            downsample_events(xs, xs, ts, ps, size, scale, T)
        with pytest.raises(ValueError, match="^t: .*" + match):
            downsample_geometry("t: ", size, scale, T)
    assert downsample_geometry("t: ", (222, 346), 4) == (222, 346, 4, 16, (56, 87))
    assert downsample_geometry("t: ", (8, 12), np.int64(3), np.int32(5)) == (8, 12, 3, 5, (3, 4))


def test_hr_entry_points_refuse_before_anything_runs():
    from event_dataset import EventTrainSet
    ds = EventTrainSet(L=3, scale=4)
    xs, ts, ps = torch.zeros(10, dtype=torch.int16), torch.arange(10, dtype=torch.float64), torch.ones(10, dtype=torch.float64)
    with pytest.raises(ValueError, match="^EventTrainSet.add_hr_recording: gt must be three tensors"):
        ds.add_hr_recording((xs, xs), ts, (8, 12))
    with pytest.raises(ValueError, match="^EventTrainSet.add_hr_recording: gt_ts must be"):
        ds.add_hr_recording((xs, xs, ps), ts.numpy(), (8, 12))
    with pytest.raises(ValueError, match="^EventTrainSet.add_hr_recording: .*GPU tensors on one device"):
        ds.add_hr_recording((xs, xs, ps), ts, (8, 12))
    for nf, match in ((dict(ts=ts, dt=0.1), "keys dt, support"), (dict(support=1), "keys dt, support"), (0.1, "keys dt, support"),
                      (dict(dt=-0.1), r"noise_filter\['dt'\]"), (dict(dt=0.1, support=9), r"noise_filter\['support'\]")):
        with pytest.raises(ValueError, match="^EventTrainSet.add_hr_recording: .*" + match):
            ds.add_hr_recording((xs, xs, ps), ts, (8, 12), noise_filter=nf)
    assert len(ds) == 0


# ------------------------------------------------------------------ 5. header, ABI text, binding, exports
NAMES = ["bmc_downsample_abi", "bmc_event_downsample_capacity", "bmc_event_downsample_chunk", "bmc_event_downsample_gather",
         "bmc_event_downsample_keys", "bmc_event_downsample_scratch_bytes", "bmc_event_downsample_walk"]


def test_companion_header_matches_its_abi_text_and_binding():
    from bmc_hip import denoise_lib, downsample_lib, lib, ssim_lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(abi_ref.INCLUDE, "bmc_hip_downsample.h")).read(), flags=re.S)
    declared = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?[a-z][a-z ]*\*?)\s*\b(bmc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, re.M):
        params = [p.strip() for p in params.split(",")]
        declared[name] = [abi_ref.classify(ret)] + ([] if params == ["void"] else [abi_ref.classify(p) for p in params])
    assert sorted(declared) == sorted(downsample_lib.FUNCTIONS) == NAMES
    for other in (lib, ssim_lib, denoise_lib):                   # the other headers' tables do not grow
        assert not set(declared) & set(other.FUNCTIONS)
    assert set(lib.EXPORTS) == set(abi_ref.functions())
    want = {"bmc_event_downsample_capacity": ["i8", "i8", "i4"], "bmc_event_downsample_chunk": ["i8", "i8"],
            "bmc_event_downsample_scratch_bytes": ["i8", "i8"],
            "bmc_event_downsample_keys": ["i4", "p", "p", "p", "i8", "i4", "i4", "i4", "p", "p", "p"],
            "bmc_event_downsample_walk": ["i4", "p", "p", "p", "i8", "i4", "i4", "i4", "i4", "p", "p"],
            "bmc_event_downsample_gather": ["i4", "p", "p", "p", "p", "i8", "i4", "p", "p", "p", "p", "i8", "p", "p", "p"]}
    for name, sig in want.items():
        assert downsample_lib.FUNCTIONS[name] == sig == declared[name], name
    assert [c.split(":")[0] for c in downsample_lib.FUNCTIONS["bmc_downsample_abi"]] == declared["bmc_downsample_abi"] == ["p"]
    kinds = {"p": C.c_void_p, "i4": C.c_int, "i8": C.c_longlong, "f8": C.c_double}
    for fn, name in ((downsample_lib._keys, "bmc_event_downsample_keys"), (downsample_lib._walk, "bmc_event_downsample_walk"),
                     (downsample_lib._gather, "bmc_event_downsample_gather")):
        assert fn.restype is C.c_int and [kinds[k] for k in want[name][1:]] == list(fn.argtypes)
    assert downsample_lib.capacity.restype is downsample_lib.scratch_bytes.restype is C.c_longlong
    assert not re.findall(r"^\}\s*(bmc_[a-z0-9_]+_t)\s*;", text, re.M)          # no struct
    names = re.findall(r"^#define[ \t]+(BMC_[A-Z0-9_]+)[ \t]+\S", text, re.M)
    assert sorted(names) == sorted(downsample_lib.CONSTANTS) == [
        "BMC_DOWNSAMPLE_LANES", "BMC_DOWNSAMPLE_LAUNCHES", "BMC_DOWNSAMPLE_MAX_PARTS", "BMC_DOWNSAMPLE_MAX_SCALE",
        "BMC_DOWNSAMPLE_MAX_THRESHOLD", "BMC_DOWNSAMPLE_TILE"]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no host C compiler"
    body = ['printf("%s %%d\\n", (int)(%s));' % (n, n) for n in names]
    src = '#include <stdio.h>\n#include "bmc_hip_downsample.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(body)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run([cc, "-I" + abi_ref.INCLUDE, os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    compiled = dict(zip(out[::2], map(int, out[1::2])))
    assert compiled == downsample_lib.CONSTANTS and all(type(v) is int for v in downsample_lib.CONSTANTS.values())
    D = downsample_lib
    assert (D.MAX_SCALE, D.MAX_THRESHOLD, D.LANES, D.TILE, D.LAUNCHES) == (16, 32767, 256, 1024, 4) and D.TILE % D.LANES == 0
    assert "bmc_hip_downsample.h" not in open(os.path.join(abi_ref.INCLUDE, "bmc_hip.h")).read()


def test_library_exports_geometry_and_refusals():
    """The symbols; capacity, chunk and scratch size as the library reports them (host code: no device needed) against the
    header's rules; the refusals of the entry points that return before anything touches a device."""
    from bmc_hip import downsample_lib as D, lib
    for name in NAMES:
        assert lib.has_symbol(name) and name not in lib.EXPORTS
    for n in (0, 1, 255, 1023, 1024, 1025, 5000, D.TILE * D.MAX_PARTS, D.TILE * D.MAX_PARTS + 1, 10 ** 7, (1 << 31) - 1):
        for T in (1, 16, 32767):
            assert D.capacity(n, T) == n // T
        per = -(-max(n, 1) // D.MAX_PARTS)
        chunk = -(-per // D.TILE) * D.TILE
        parts = max(1, -(-n // chunk))
        assert D.chunk(n) == chunk and parts <= D.MAX_PARTS and D.scratch_bytes(n) == -(-4 * parts // 8) * 8
    assert (D.chunk(0), D.chunk(2 * D.TILE * D.MAX_PARTS), D.scratch_bytes(1)) == (D.TILE, 2 * D.TILE, 8)
    for n, T in ((-1, 1), (1 << 31, 1), (5, 0), (5, 32768)):
        assert D.capacity(n, T) == -1
    assert D.chunk(-1) == D.chunk(1 << 31) == D.scratch_bytes(-1) == D.scratch_bytes(1 << 31) == -1
    p = 4096                                                 # never dereferenced: every call below returns at its argument check
    keys = dict(xs=p, ys=p, ps=p, n=4, H=5, W=7, s=2, keys=p, fire=p, st=None)
    for kw in (dict(n=1 << 31), dict(n=-1), dict(H=0), dict(W=0), dict(s=0), dict(s=17), dict(xs=None), dict(ys=None), dict(ps=None),
               dict(keys=None), dict(fire=None), dict(H=1 << 16, W=1 << 16, s=1), dict(H=46341, W=46341, s=1)):
        assert D._keys(*{**keys, **kw}.values()) == -1 and b"bmc_event_downsample_keys" in lib.bmc_last_error(), kw
    walk = dict(sorted=p, perm=p, ps=p, n=4, H=5, W=7, s=2, T=4, fire=p, st=None)
    for kw in (dict(n=1 << 31), dict(n=-1), dict(H=0), dict(W=0), dict(s=0), dict(s=17), dict(T=0), dict(T=32768), dict(sorted=None),
               dict(perm=None), dict(ps=None), dict(fire=None), dict(H=1 << 16, W=1 << 16, s=1)):
        assert D._walk(*{**walk, **kw}.values()) == -1 and b"bmc_event_downsample_walk" in lib.bmc_last_error(), kw
    gather = dict(xs=p, ys=p, ts=p, fire=p, n=4, s=2, oxs=p, oys=p, ots=p, ops=p, cap=1, count=p, scratch=p, st=None)
    for kw in (dict(n=1 << 31), dict(n=-1), dict(s=0), dict(s=17), dict(cap=-1), dict(count=None), dict(scratch=None),
               dict(scratch=p + 4), dict(xs=None), dict(ys=None), dict(ts=None), dict(fire=None), dict(oxs=None), dict(oys=None),
               dict(ots=None), dict(ops=None)):
        assert D._gather(*{**gather, **kw}.values()) == -1 and b"bmc_event_downsample_gather" in lib.bmc_last_error(), kw


def test_makefile_names_the_source_once_and_the_header_as_a_dependency():
    mk = open(os.path.join(ROOT, "bmcnet-esr_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert srcs.count("event_downsample.hip") == 1 and mk.count("event_downsample.hip") == 1 and len(srcs) == len(set(srcs))
    assert mk.count("../../include/bmc_hip_downsample.h") == 1
    abi = open(os.path.join(ROOT, "bmcnet-esr_amd", "csrc", "abi.hip")).read()
    assert abi.count('#include "bmc_hip_downsample.h"') == 1


def test_tools_know_the_option():
    tools = os.path.join(ROOT, "tools")
    assert '"--from-hr"' in open(os.path.join(tools, "multistream_infer.py")).read()
    assert '"--from-hr"' in open(os.path.join(tools, "train_events.py")).read()
    assert "downsample_grouped" in open(os.path.join(tools, "time_downsample.py")).read()


# ------------------------------------------------------------------ 6. the compiler's figures
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch_and_the_gathers_lds_fits(tmp_path):
    """Four kernels, none keeps anything in scratch memory.  Static LDS: keys and walk none; the totals four uint32; the write
    launch the staged indices of a tile, the (round, wave) counts and sum_parts' four uint64."""
    from test_isa_hygiene import CSRC, _kernels
    from bmc_hip import downsample_lib as D
    o = os.path.join(tmp_path, "event_downsample.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", o, os.path.join(CSRC, "event_downsample.hip")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    ks = {n: k for n, k in _kernels(o).items() if "NumVgprs" in k}
    want = ("event_downsample_keys_kernel", "event_downsample_walk_kernel", "event_downsample_total_kernel",
            "event_downsample_write_kernel")
    assert len(ks) == 4 and all(any(w in n for n in ks) for w in want), sorted(ks)
    for n, k in ks.items():
        assert k["ScratchSize"] == 0, (n, k)
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", open(o).read())]
    assert sorted(lds) == [0, 0, 16, 4 * D.TILE + 4 * (D.TILE // D.LANES) * 4 + 32] and max(lds) <= 65536
