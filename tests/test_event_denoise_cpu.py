"""The background-activity noise filter without a GPU: the two restatements of tests/event_denoise_ref.py against each other and
against hand-written expectations, the refusals of bmc_hip.encodings.check_noise_filter, the companion header
include/bmc_hip_denoise.h against the library's ABI text, a C compile and the binding, the exports, and the compiler's figures
for csrc/event_denoise.hip (LDS bytes, no scratch)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import abi_ref
import event_denoise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------ 1. the two restatements
SIZES = {(1, 1): (300, 0.2), (1, 9): (200, 2e-2), (5, 7): (600, 2e-2), (37, 53): (6000, 1e-2), (64, 96): (20000, 5e-3)}


@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("H,W", list(SIZES))
def test_sequential_and_sorted_forms_agree_on_every_event(H, W, k):
    n, dt = SIZES[H, W]
    for noise, dt_ in ((0.3, dt), (1.0, 10.0)):              # the drifting bar; a dense stream, where support 8 is reached
        xs, ys, ts, ps = R.stream(H, W, n, noise, seed=H * W + n + 1)
        oob = (xs < 0) | (xs >= W) | (ys < 0) | (ys >= H)
        assert n < 6000 or all((c < 0).any() and (c >= m).any() for c, m in ((xs, W), (ys, H)))          # out of range on every side
        assert (np.diff(ts) >= 0).all() and (n < 6000 or (np.diff(ts) == 0).any())                      # sorted, with ties
        a = R.mask_seq(xs, ys, ts, H, W, dt_, k)
        b = R.mask_sorted(torch.tensor(xs), torch.tensor(ys), torch.tensor(ts), H, W, dt_, k)
        assert a.dtype == np.uint8 and b.dtype == torch.uint8 and np.array_equal(a, b.numpy())
        assert not a[oob].any()
        if (H, W) != (1, 1) and noise == 0.3 and k <= 2:
            assert 0.05 <= a.mean() <= 0.95, a.mean()        # both outcomes occur
        if k == 8 and noise == 1.0:
            assert (0 < a.sum() < n) == (H >= 3 and W >= 3)  # the full ring exists only inside a sensor of 3 x 3 or more


def test_generated_cases_keep_and_drop():
    """The kept shares of the generated GPU cases, on the restatement alone: [0.05, 0.95] for support 1 and 2."""
    for (H, W, n), dt in R.CASES.items():
        xs, ys, ts, _ = R.stream(H, W, n, 0.3, seed=H * W + n + 1)
        for k in (1, 2):
            keep = R.mask_seq(xs, ys, ts, H, W, dt, k)
            print(H, W, n, dt, k, "kept share %.3f" % keep.mean())
            assert R.both_outcomes(keep, n)


# ------------------------------------------------------------------ 2. planted streams
def _both(xs, ys, ts, H, W, dt, k):
    a = R.mask_seq(np.array(xs), np.array(ys), np.array(ts, np.float64), H, W, dt, k)
    b = R.mask_sorted(torch.tensor(xs), torch.tensor(ys), torch.tensor(ts, dtype=torch.float64), H, W, dt, k)
    assert np.array_equal(a, b.numpy())
    return a.tolist()


def test_planted_streams():
    H, W = 5, 7
    assert _both([3], [2], [0.5], H, W, 1.0, 1) == [0]                                           # a lone event
    d = 0.3 - 0.1
    assert _both([3, 4], [2, 2], [0.1, 0.3], H, W, d, 1) == [0, 1]                               # dt apart: the second only
    assert _both([3, 4], [2, 2], [0.1, 0.3], H, W, float(np.nextafter(d, 0.0)), 1) == [0, 0]     # one ulp more than dt apart
    assert _both([3, 4, 3], [2, 3, 2], [0.7, 0.7, 0.7], H, W, 0.0, 1) == [0, 1, 1]               # ties: column order only
    assert _both([3, 3, 3], [2, 2, 2], [0.1, 0.1, 0.2], H, W, 1.0, 1) == [0, 0, 0]               # the pixel itself never counts
    ring = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
    for cx, cy, want in ((3, 2, 1), (0, 0, 0), (6, 4, 0), (0, 2, 0)):                            # support 8: the full ring ...
        xs, ys = [cx + dx for dx, _ in ring] + [cx], [cy + dy for _, dy in ring] + [cy]          # ... fails at a corner, an edge
        assert _both(xs, ys, [0.01 * i for i in range(9)], H, W, 1.0, 8)[-1] == want
        assert _both(xs, ys, [0.01 * i for i in range(9)], H, W, 1.0, 3)[-1] == 1
    assert _both(xs[1:], ys[1:], [0.01 * i for i in range(8)], H, W, 1.0, 8)[-1] == 0            # seven of eight
    assert _both([1, 2, 3, 4], [1, 1, 1, 1], [0.1, 0.1, 0.2, 0.2], H, W, 0.0, 1) == [0, 1, 0, 1]  # dt = 0: only ties support
    assert _both([3, -1, 4], [2, 2, 2], [0.1, 0.2, 0.3], H, W, 1.0, 1) == [0, 0, 1]
    assert _both([W, 6], [2, 2], [0.1, 0.2], H, W, 1.0, 1) == [0, 0]                             # out of range: no support ...
    assert _both([6, W], [2, 2], [0.1, 0.2], H, W, 1.0, 1) == [0, 0]                             # ... and no survival
    assert _both([3, 3], [-1, 0], [0.1, 0.2], H, W, 1.0, 1) == [0, 0] == _both([3, 3], [H, H - 1], [0.1, 0.2], H, W, 1.0, 1)
    assert _both([0, 6], [1, 0], [0.1, 0.2], H, W, 1.0, 1) == [0, 0]                             # rows do not wrap around
    assert _both([], [], [], H, W, 1.0, 1) == []


# ------------------------------------------------------------------ 3. check_noise_filter
def test_check_noise_filter_refusals():
    from bmc_hip import denoise_lib
    from bmc_hip.encodings import check_noise_filter
    ts = torch.arange(10, dtype=torch.float64)
    assert check_noise_filter("t: ", None) is None
    got = check_noise_filter("t: ", dict(ts=ts, dt=0.5))
    assert got[0] is ts and got[1:] == (0.5, 1) and check_noise_filter("t: ", dict(ts=ts, dt=0, support=8))[1:] == (0.0, 8)
    for bad, match in ((0.5, "must be None or a dict"), (dict(ts=ts, dt=0.5, window=3), "unknown key 'window'"),
                       (dict(ts=ts), "lacks the key 'dt'"), (dict(dt=0.5), "lacks the key 'ts'"),
                       (dict(ts=ts, dt=-1e-9), r"\['dt'\]"), (dict(ts=ts, dt=math.inf), r"\['dt'\]"), (dict(ts=ts, dt=math.nan), r"\['dt'\]"),
                       (dict(ts=ts, dt="1"), r"\['dt'\]"), (dict(ts=ts, dt=True), r"\['dt'\]"), (dict(ts=ts, dt=0.5, support=0), r"\['support'\]"),
                       (dict(ts=ts, dt=0.5, support=9), r"\['support'\]"), (dict(ts=ts, dt=0.5, support=2.0), r"\['support'\]"),
                       (dict(ts=ts.float(), dt=0.5), r"\['ts'\]"), (dict(ts=ts.numpy(), dt=0.5), r"\['ts'\]"),
                       (dict(ts=ts.view(2, 5), dt=0.5), r"\['ts'\]"), (dict(ts=ts.flip(0), dt=0.5), "finite and non-decreasing"),
                       (dict(ts=torch.tensor([0.0, math.nan], dtype=torch.float64), dt=0.5), "finite and non-decreasing"),
                       (dict(ts=torch.tensor([0.0, math.inf], dtype=torch.float64), dt=0.5), "finite and non-decreasing")):
        with pytest.raises(ValueError, match="^t: .*" + match):
            check_noise_filter("t: ", bad)
    xs, ps = torch.zeros(10, dtype=torch.int16), torch.zeros(10)
    for cols, size, match in (((xs, xs, ps.double()), (5, 7), "GPU tensors on one device"), ((xs, xs.int(), ps.double()), (5, 7), "ys must be"),
                              ((xs, xs, ps), (5, 7), "ps must be"), ((xs[:9], xs[:9], ps.double()[:9]), (5, 7), "ts has 10 entries, xs 9"),
                              (None, (5, denoise_lib.MAX_W + 1), "at most %d wide" % denoise_lib.MAX_W), (None, (0, 7), "must be positive"),
                              (None, 7, r"sensor_size = \(H, W\)")):
        with pytest.raises(ValueError, match=match):
            check_noise_filter("t: ", dict(ts=ts, dt=0.5), cols, size)


# ------------------------------------------------------------------ 4. header, ABI text, binding; 5. exports
def test_companion_header_matches_its_abi_text_and_binding():
    from bmc_hip import denoise_lib, lib, ssim_lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(abi_ref.INCLUDE, "bmc_hip_denoise.h")).read(), flags=re.S)
    declared = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?[a-z][a-z ]*\*?)\s*\b(bmc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, re.M):
        params = [p.strip() for p in params.split(",")]
        declared[name] = [abi_ref.classify(ret)] + ([] if params == ["void"] else [abi_ref.classify(p) for p in params])
    assert sorted(declared) == sorted(denoise_lib.FUNCTIONS) == ["bmc_denoise_abi", "bmc_event_denoise", "bmc_event_denoise_band_rows",
                                                                "bmc_event_denoise_scratch_bytes"]
    for other in (lib, ssim_lib):                            # the other headers' tables do not grow
        assert not set(declared) & set(other.FUNCTIONS)
    assert set(lib.EXPORTS) == set(abi_ref.functions())
    want = ["i4", "p", "p", "p", "p", "i8", "i4", "i4", "f8", "i4", "p", "p", "p", "p", "p"]
    assert denoise_lib.FUNCTIONS["bmc_event_denoise"] == want == declared["bmc_event_denoise"]
    assert denoise_lib.FUNCTIONS["bmc_event_denoise_band_rows"] == ["i4", "i4", "i4"] == declared["bmc_event_denoise_band_rows"]
    assert denoise_lib.FUNCTIONS["bmc_event_denoise_scratch_bytes"] == ["i8", "i4", "i4"] == declared["bmc_event_denoise_scratch_bytes"]
    assert [c.split(":")[0] for c in denoise_lib.FUNCTIONS["bmc_denoise_abi"]] == declared["bmc_denoise_abi"] == ["p"]
    kinds = {"p": C.c_void_p, "i4": C.c_int, "i8": C.c_longlong, "f8": C.c_double}
    assert denoise_lib._event_denoise.restype is C.c_int and [kinds[k] for k in want[1:]] == list(denoise_lib._event_denoise.argtypes)
    assert denoise_lib.scratch_bytes.restype is C.c_longlong
    assert not re.findall(r"^\}\s*(bmc_[a-z0-9_]+_t)\s*;", text, re.M)          # no struct
    names = re.findall(r"^#define[ \t]+(BMC_[A-Z0-9_]+)[ \t]+\S", text, re.M)
    assert sorted(names) == sorted(denoise_lib.CONSTANTS) == ["BMC_DENOISE_LDS_WORDS", "BMC_DENOISE_MAX_W", "BMC_DENOISE_STEP"]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no host C compiler"
    body = ['printf("%s %%d\\n", (int)(%s));' % (n, n) for n in names]
    src = '#include <stdio.h>\n#include "bmc_hip_denoise.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(body)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run([cc, "-I" + abi_ref.INCLUDE, os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    compiled = dict(zip(out[::2], map(int, out[1::2])))
    assert compiled == denoise_lib.CONSTANTS and all(type(v) is int for v in denoise_lib.CONSTANTS.values())
    S, L, MW = denoise_lib.STEP, denoise_lib.LDS_WORDS, denoise_lib.MAX_W
    assert (S, L) == (256, 15360) and MW >= 1280 and L // (MW + 2) - 2 >= 1       # a band of the widest sensor has a row to own
    assert "bmc_hip_denoise.h" not in open(os.path.join(abi_ref.INCLUDE, "bmc_hip.h")).read()


def test_library_exports_and_band_geometry():
    """The symbols; the band height and scratch size the library reports (host code: no device needed) against the header's rule;
    the refusals of the entry point that return before anything touches a device."""
    from bmc_hip import denoise_lib, lib
    for name in ("bmc_event_denoise", "bmc_event_denoise_band_rows", "bmc_event_denoise_scratch_bytes", "bmc_denoise_abi"):
        assert lib.has_symbol(name) and name not in lib.EXPORTS
    L, MW = denoise_lib.LDS_WORDS, denoise_lib.MAX_W
    for H, W in ((1, 1), (1, 9), (5, 7), (37, 53), (180, 240), (720, 1280), (7, MW), (32767, MW), (260, 346), (480, 640)):
        r = denoise_lib.band_rows(H, W)
        assert r == min(H, L // (W + 2) - 2) >= 1 and (r + 2) * (W + 2) <= L
        assert denoise_lib.scratch_bytes(H, W) == 8 * -(-H // r)
    assert (denoise_lib.band_rows(180, 240), denoise_lib.band_rows(720, 1280), denoise_lib.band_rows(7, MW)) == (61, 9, 3)
    for H, W in ((0, 7), (5, 0), (5, MW + 1), (-1, -1)):
        assert denoise_lib.band_rows(H, W) == -1 == denoise_lib.scratch_bytes(H, W)
    p = 4096                                                 # never dereferenced: every call below returns at its argument check
    good = dict(xs=p, ys=p, ts=p, ps=p, n=4, H=5, W=7, dt=0.1, k=1, keep=p, ps_out=p, kept=p, scratch=p, s=None)
    for kw in (dict(n=1 << 31), dict(n=-1), dict(W=MW + 1), dict(W=0), dict(H=0), dict(k=0), dict(k=9), dict(dt=-1e-9), dict(dt=math.inf),
               dict(dt=math.nan), dict(xs=None), dict(ys=None), dict(ts=None), dict(ps=None), dict(scratch=None), dict(scratch=p + 4)):
        assert denoise_lib._event_denoise(*{**good, **kw}.values()) == -1 and b"bmc_event_denoise" in lib.bmc_last_error(), kw


def test_makefile_names_the_source_once_and_the_header_as_a_dependency():
    mk = open(os.path.join(ROOT, "bmcnet-esr_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert srcs.count("event_denoise.hip") == 1 and mk.count("event_denoise.hip") == 1 and len(srcs) == len(set(srcs))
    assert mk.count("../../include/bmc_hip_denoise.h") == 1
    abi = open(os.path.join(ROOT, "bmcnet-esr_amd", "csrc", "abi.hip")).read()
    assert abi.count('#include "bmc_hip_denoise.h"') == 1


def test_tools_know_the_option():
    tools = os.path.join(ROOT, "tools")
    assert '"--noise-filter"' in open(os.path.join(tools, "multistream_infer.py")).read()
    assert '"--denoise"' in open(os.path.join(tools, "train_events.py")).read()
    assert "mask_sorted" in open(os.path.join(tools, "time_denoise.py")).read()


# ------------------------------------------------------------------ 6. the compiler's figures
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch_and_their_lds_fits(tmp_path):
    """Two kernels, neither keeps anything in scratch memory.  Static LDS of the band kernel: the surface, the step's pixel
    list and the four waves' counts -- under 64 KB; of the finish launch four int64."""
    from test_isa_hygiene import CSRC, _kernels
    from bmc_hip import denoise_lib
    o = os.path.join(tmp_path, "event_denoise.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", o, os.path.join(CSRC, "event_denoise.hip")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    ks = {n: k for n, k in _kernels(o).items() if "NumVgprs" in k}
    want = ("event_denoise_kernel", "event_denoise_finish_kernel")
    assert len(ks) == 2 and all(any(w in n for n in ks) for w in want), sorted(ks)
    for n, k in ks.items():
        assert k["ScratchSize"] == 0, (n, k)
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", open(o).read())]
    assert sorted(lds) == [32, 4 * (denoise_lib.LDS_WORDS + denoise_lib.STEP + 4)] and max(lds) <= 65536
