"""The structural training loss (include/bmc_hip_ssim.h), the parts that need no GPU: tests/ssim_loss_ref.py's ordered
restatement against float64 autograd of the conv2d formulation and against tests/quality_ref.py's SSIM; losses.SSIM / Mix as
plain torch on CPU tensors; their refusals; losses.parse; the routing predicates; the companion header against the library's ABI
text and the binding; the entry points' refusals; the Makefile; the compiler's figures for the three kernels."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import quality_ref as Q
import ssim_loss_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SHAPES = [(7, 7), (9, 13), (40, 70)]
RANGES = [1.0, 8.0, 255.0]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------ the oracle
def test_restatement_gradient_equals_float64_autograd():
    """The closed form (three coefficients per position, gathered) is the gradient of the conv2d formulation: the two float64
    evaluations differ by rounding only.  n terms of magnitude up to 255^2 cancel to C2 = (0.03 R)^2 at R = 1, so the distance
    in a relative L2 sense is bounded by a few thousand u = 2^-53, not by u: 1e-11 is asserted, 4e-16 .. 1e-13 measured."""
    for h, w in SHAPES:
        for R in RANGES:
            x, y = SR.make_pair(2, 2, h, w, seed=h * 100 + w)
            L, g = SR.conv2d_loss_and_grad(x, y, R)
            g2 = SR.grad(x, y, R)
            assert g2.shape == g.shape == x.shape and g2.dtype == np.float64
            print("%dx%d R=%g loss %.15f / %.15f  gradient rel-L2 %.2e" % (h, w, R, SR.loss(x, y, R), L, _rel(g2, g)))
            assert abs(SR.loss(x, y, R) - L) <= 1e-12
            assert _rel(g2, g) <= 1e-11
            assert np.array_equal(SR.grad(x, y, R, 0.375), g2 * 0.375)          # a power-of-two-free scale is applied last
    # dense counts: the regime the float64 requirement is for
    r = np.random.default_rng(3)
    y = r.integers(0, 256, (1, 2, 12, 15)).astype(np.float32)
    x = (y + r.standard_normal(y.shape)).astype(np.float32)
    L, g = SR.conv2d_loss_and_grad(x, y, 255.0)
    assert abs(SR.loss(x, y, 255.0) - L) <= 1e-12 and _rel(SR.grad(x, y, 255.0), g) <= 1e-11


def test_one_minus_loss_is_the_quality_oracles_ssim():
    for h, w in SHAPES + [(39, 137)]:
        for R in RANGES:
            x, y = SR.make_pair(1, 2, h, w, seed=h + w)
            _, ssim = Q.quality(x, y, R)
            assert abs((1.0 - SR.loss(x, y, R)) - ssim[0]) <= Q.SSIM_BAR, (h, w, R)


def test_exact_cases_of_the_restatement():
    x, y = SR.make_pair(2, 2, 9, 13, seed=1)
    assert SR.loss(y, y, 8.0) == 0.0 and not SR.grad(y, y, 8.0).any()
    z = np.zeros((1, 2, 8, 9), np.float32)
    assert SR.loss(z, z, 1.0) == 0.0 and not SR.grad(z, z, 1.0).any()
    a, b, g = SR.coefficients(z, z, 1.0)
    assert not a.any() and (b > 0).all() and np.array_equal(b, -g)      # beta and gamma multiply y = x = 0


def test_tile_partials_add_up_in_any_tiling():
    S = np.random.default_rng(0).random((3, 45, 150))
    for TH in (4, 32):
        p = SR.tile_partials(S, TH, 64)
        assert p.shape == (3, -(-45 // TH) * 3) and abs(p.sum() - S.sum()) <= 1e-9


# ------------------------------------------------------------------ losses.SSIM / Mix as plain torch
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_loss_objects_on_cpu_tensors_equal_the_restatement(dtype):
    from bmc_hip import losses
    for h, w in SHAPES:
        for R in (1.0, 8.0):
            x, y = SR.make_pair(2, 2, h, w, seed=7 * h + w)
            xt, yt = torch.tensor(x).to(dtype).requires_grad_(), torch.tensor(y).to(dtype)
            want, gwant = SR.loss(x, y, R), SR.grad(x, y, R)
            # the result is rounded to the inputs' dtype once: half an ulp of it, plus the two float64 orders' distance
            eps = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
            got = losses.SSIM(R)(xt, yt)
            assert got.dtype == dtype and got.dim() == 0
            assert abs(float(got.detach()) - want) <= eps * abs(want) + 1e-12
            (g,) = torch.autograd.grad(got, xt)
            assert g.dtype == dtype and _rel(g.double().numpy(), gwant) <= (1e-6 if dtype == torch.float32 else 1e-11)
            for point, ref in ((None, F.mse_loss), (losses.L1(), F.l1_loss), (losses.Huber(0.5), lambda a, b: F.huber_loss(a, b, delta=0.5))):
                m = losses.Mix(point, losses.SSIM(R), 0.25)
                pw = float(ref(xt.detach().double(), yt.double()))
                # the pointwise mean is taken in the inputs' dtype: a pairwise sum of n terms, (log2 n + 4) half-ulps at most
                bar = (math.log2(x.size) + 4) * eps * abs(pw) + 4 * eps * (abs(pw) + abs(want)) + 1e-12
                assert abs(float(m(xt.detach(), yt)) - (0.75 * pw + 0.25 * want)) <= bar
    assert float(losses.Mix(losses.L1(), losses.SSIM())(yt, yt)) == 0.0


def test_loss_object_parameters_and_refusals():
    from bmc_hip import losses
    s = losses.SSIM()
    assert (s.kind, s.name, s.param, repr(s)) == ("ssim", "ssim", 1.0, "SSIM(1)") and losses.SSIM(8).param == 8.0
    assert type(losses.SSIM(np.float32(2.5)).param) is float
    for bad in (0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="data_range"):
            losses.SSIM(bad)
    m = losses.Mix(None, s)
    assert (m.pointwise, m.structural, m.alpha, m.name) == (None, s, 0.84, "mse+ssim")
    assert losses.Mix(losses.Huber(2.0), s, 0.5).name == "huber+ssim"
    for bad in (0.0, 1.0, -0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="alpha"):
            losses.Mix(None, s, bad)
    for bad in (F.l1_loss, s, "l1", losses.Mix(None, s)):
        with pytest.raises(TypeError, match="pointwise"):
            losses.Mix(bad, s)
    for bad in (None, losses.L1(), F.mse_loss, "ssim"):
        with pytest.raises(TypeError, match="structural"):
            losses.Mix(losses.L1(), bad)
    with pytest.raises(ValueError, match="h, w >= 7"):
        s(torch.zeros(1, 2, 6, 9), torch.zeros(1, 2, 6, 9))
    with pytest.raises(ValueError, match="one shape"):
        s(torch.zeros(1, 2, 8, 9), torch.zeros(1, 2, 9, 9))


def test_routing_predicates():
    from bmc_hip import losses
    s, m = losses.SSIM(), losses.Mix(losses.L1(), losses.SSIM(4.0))
    assert not losses.is_fusable(s) and not losses.is_fusable(m)                     # ops.head_loss refuses them
    assert losses.is_structural(s) and losses.is_structural(m) and losses.on_device_path(s) and losses.on_device_path(m)
    for p in (losses.L1(), losses.Huber(), losses.Charbonnier()):
        assert losses.is_fusable(p) and not losses.is_structural(p) and losses.on_device_path(p)
    for other in (None, F.mse_loss, F.l1_loss, losses.SSIM, (lambda a, b: s(a, b)), "ssim"):
        assert not losses.is_structural(other) and not losses.on_device_path(other)
    with pytest.raises(TypeError, match="not a bmc_hip.losses object"):
        from bmc_hip import ops
        ops.head_loss(torch.zeros(1, 1, 1, 4), torch.zeros(1, 1, 1, 1), torch.zeros(1, 1, 2, 2), 2, s)


def test_parse_new_forms_and_everything_refused_before():
    from bmc_hip import losses
    assert losses.parse("mse") is None and type(losses.parse("l1")) is losses.L1
    assert losses.parse("huber:2").param == 2.0 and losses.parse("huber:1e+3").param == 1000.0
    s = losses.parse("ssim")
    assert type(s) is losses.SSIM and s.param == 1.0 and losses.parse("SSIM:8").param == 8.0 and losses.parse(" ssim:0.5 ").param == 0.5

    def mix(spec):
        m = losses.parse(spec)
        assert type(m) is losses.Mix
        p = m.pointwise
        return (None if p is None else (p.name, p.param)), m.structural.param, m.alpha

    assert mix("l1+ssim:8@0.84") == (("l1", 0.0), 8.0, 0.84)
    assert mix("mse+ssim") == (None, 1.0, 0.84)
    assert mix("huber+ssim@0.5") == (("huber", 1.0), 1.0, 0.5)
    assert mix("huber:0.25+ssim:4") == (("huber", 0.25), 4.0, 0.84)
    assert mix("charbonnier:1e-2 + ssim:255@0.1") == (("charbonnier", 0.01), 255.0, 0.1)
    assert mix("huber:1e+3+ssim:1e+1@5e-1") == (("huber", 1000.0), 10.0, 0.5)
    for bad in ("l2", "huber:0", "mse:1", "l1:2", "huber:x", "charbonnier:-1", "", "l1_loss", "huber:inf",                 # as before
                "ssim:0", "ssim:-1", "ssim:x", "ssim:inf", "ssim@0.5", "ssim+l1", "ssim+ssim", "l2+ssim", "l1:2+ssim", "mse:1+ssim",
                "huber:0+ssim", "l1+ssim@", "l1+ssim@0", "l1+ssim@1", "l1+ssim@x", "l1+ssim:0", "l1+ssim:8@0.5@0.5", "l1+msssim",
                "l1+", "+ssim"):
        with pytest.raises(ValueError):
            losses.parse(bad)
    with pytest.raises(ValueError, match=r"ssim\[:R\].*POINT\+ssim\[:R\]\[@ALPHA\]"):
        losses.parse("l2")


def test_ops_ssim_loss_refuses_cpu_tensors_and_bad_ranges():
    from bmc_hip import ops
    a = torch.zeros(1, 2, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ssim_loss(a, a, 1.0)
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="data_range"):
            ops.ssim_loss(a, a, bad)


def test_tools_know_the_new_specs():
    for tool in ("train_events.py", "time_head_loss.py"):
        src = open(os.path.join(ROOT, "tools", tool)).read()
        assert "losses.parse" in src and "ssim" in src, tool


# ------------------------------------------------------------------ the companion header and its binding
def test_companion_header_matches_its_abi_text_and_binding():
    """include/bmc_hip_ssim.h by the routes tests/test_quality_cpu.py takes for bmc_hip_quality.h: the header's text and a C
    compile of it, against bmc_ssim_abi() and what bmc_hip/ssim_lib.py installs."""
    import ctypes as C
    import shutil
    import tempfile
    import abi_ref
    from bmc_hip import lib, loss_lib, quality_lib, ssim_lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(abi_ref.INCLUDE, "bmc_hip_ssim.h")).read(), flags=re.S)
    declared = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?[a-z][a-z ]*\*?)\s*\b(bmc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, re.M):
        params = [p.strip() for p in params.split(",")]
        declared[name] = [abi_ref.classify(ret)] + ([] if params == ["void"] else [abi_ref.classify(p) for p in params])
    assert sorted(declared) == sorted(ssim_lib.FUNCTIONS) == ["bmc_ssim_abi", "bmc_ssim_loss_bwd", "bmc_ssim_loss_fwd"]
    for other in (lib, loss_lib, quality_lib):                      # the other headers' tables do not grow
        assert not set(declared) & set(other.FUNCTIONS)
    # struct-free argument codes: pointers, int, long long, double only, and exactly the header's
    assert ssim_lib.FUNCTIONS["bmc_ssim_loss_fwd"] == ["i4", "p", "p", "i8", "i4", "i4", "i4", "i4", "f8", "p", "p", "p"] == declared["bmc_ssim_loss_fwd"]
    assert ssim_lib.FUNCTIONS["bmc_ssim_loss_bwd"] == ["i4", "p", "p", "i8", "p", "i4", "i4", "i4", "i4", "f8", "p", "p"] == declared["bmc_ssim_loss_bwd"]
    assert [c.split(":")[0] for c in ssim_lib.FUNCTIONS["bmc_ssim_abi"]] == declared["bmc_ssim_abi"] == ["p"]
    kinds = {"p": C.c_void_p, "i4": C.c_int, "i8": C.c_longlong, "f8": C.c_double}
    for name, fn in (("bmc_ssim_loss_fwd", ssim_lib._ssim_loss_fwd), ("bmc_ssim_loss_bwd", ssim_lib._ssim_loss_bwd)):
        assert fn.restype is C.c_int and [kinds[k] for k in declared[name][1:]] == list(fn.argtypes)
    assert not re.findall(r"^\}\s*(bmc_[a-z0-9_]+_t)\s*;", text, re.M)          # no struct
    names = re.findall(r"^#define[ \t]+(BMC_[A-Z0-9_]+)[ \t]+\S", text, re.M)
    assert sorted(names) == sorted(ssim_lib.CONSTANTS) == ["BMC_SSIM_BWD_TILE_H", "BMC_SSIM_BWD_TILE_W", "BMC_SSIM_TILE_H",
                                                           "BMC_SSIM_TILE_W", "BMC_SSIM_WIN"]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no host C compiler"
    body = ['printf("%s %%d\\n", (int)(%s));' % (n, n) for n in names]
    src = '#include <stdio.h>\n#include "bmc_hip_ssim.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(body)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run([cc, "-I" + abi_ref.INCLUDE, os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    compiled = dict(zip(out[::2], map(int, out[1::2])))
    assert compiled == ssim_lib.CONSTANTS and all(type(v) is int for v in ssim_lib.CONSTANTS.values())
    assert compiled["BMC_SSIM_WIN"] == 7 == quality_lib.const("BMC_QUALITY_WIN")
    TH, TW, PH, PW = ssim_lib.TILE_H, ssim_lib.TILE_W, ssim_lib.BWD_TILE_H, ssim_lib.BWD_TILE_W
    assert (TH, TW, PH, PW) == tuple(compiled["BMC_SSIM_" + k] for k in ("TILE_H", "TILE_W", "BWD_TILE_H", "BWD_TILE_W"))
    assert TW == 64 and TH % 4 == 0 and PW == 32 and PH * PW == 512                  # what the kernels' thread maps assume
    assert 2 * (PH + 12) * (PW + 12) * 4 + 3 * (PH + 6) * (PW + 6) * 8 <= 65536      # the backward's static LDS
    assert ssim_lib.fwd_tiles(7, 7) == 1 and ssim_lib.fwd_tiles(TH + 6, TW + 6) == 1 and ssim_lib.fwd_tiles(TH + 7, TW + 7) == 4
    assert ssim_lib.fwd_tiles(2 * TH + 9, 3 * TW + 11) == 12 and (ssim_lib.FWD_LAUNCHES, ssim_lib.BWD_LAUNCHES) == (2, 1)
    assert lib.has_symbol("bmc_ssim_loss_fwd") and lib.has_symbol("bmc_ssim_loss_bwd") and lib.has_symbol("bmc_ssim_abi")
    assert "bmc_hip_ssim.h" not in open(os.path.join(abi_ref.INCLUDE, "bmc_hip.h")).read()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from bmc_hip import lib, ssim_lib
    p = 4096                                                 # never dereferenced: every call below returns at its argument check
    fwd = dict(x=p, y=p, ybs=2 * 9 * 12, B=3, C=2, h=9, w=12, R=1.0, tiles=p, loss=p, s=None)
    bwd = dict(x=p, y=p, ybs=2 * 9 * 12, gloss=p, B=3, C=2, h=9, w=12, R=1.0, dx=p, s=None)
    common = (dict(x=None), dict(y=None), dict(h=6), dict(w=6), dict(B=0), dict(C=0), dict(B=1 << 10, C=1 << 10, h=32, w=32, ybs=1 << 20),
              dict(B=1 << 15, C=1 << 15, h=7, w=7, ybs=1 << 30), dict(R=0.0), dict(R=-1.0), dict(R=math.inf), dict(R=math.nan),
              dict(ybs=2 * 9 * 12 - 1), dict(ybs=0), dict(ybs=-216))
    for kw in common + (dict(tiles=None), dict(loss=None), dict(tiles=p + 4), dict(B=1 << 12, C=1 << 11, h=7, w=7, ybs=49 << 11)):
        assert ssim_lib._ssim_loss_fwd(*{**fwd, **kw}.values()) == -1 and b"bmc_ssim_loss_fwd" in lib.bmc_last_error(), kw
    for kw in common + (dict(gloss=None), dict(dx=None), dict(B=1 << 12, C=1 << 11, h=7, w=7, ybs=49 << 11)):
        assert ssim_lib._ssim_loss_bwd(*{**bwd, **kw}.values()) == -1 and b"bmc_ssim_loss_bwd" in lib.bmc_last_error(), kw


def test_makefile_names_the_source_once_and_the_header_as_a_dependency():
    mk = open(os.path.join(ROOT, "bmcnet-esr_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert srcs.count("ssim_loss.hip") == 1 and mk.count("ssim_loss.hip") == 1 and len(srcs) == len(set(srcs))
    assert mk.count("../../include/bmc_hip_ssim.h") == 1
    abi = open(os.path.join(ROOT, "bmcnet-esr_amd", "csrc", "abi.hip")).read()
    assert abi.count('#include "bmc_hip_ssim.h"') == 1


# ------------------------------------------------------------------ the compiler's figures
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_use_no_scratch_and_their_lds_fits(tmp_path):
    """Three kernels; none keeps anything in scratch memory; static LDS: the tile launch 2 x (TH + 6) x 72 floats (+ the waves'
    sums), the gradient launch two staged images and three coefficient maps, both far inside the 64 KB a workgroup may own."""
    from test_isa_hygiene import CSRC, _kernels
    from bmc_hip import ssim_lib
    o = os.path.join(tmp_path, "ssim_loss.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                        "--cuda-device-only", "-o", o, os.path.join(CSRC, "ssim_loss.hip")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    ks = {n: k for n, k in _kernels(o).items() if "NumVgprs" in k}
    want = ("ssim_tiles_kernel", "ssim_finish_kernel", "ssim_grad_kernel")
    assert len(ks) == 3 and all(any(w in n for n in ks) for w in want), sorted(ks)
    for n, k in ks.items():
        assert k["ScratchSize"] == 0 and k["Occupancy"] >= 2, (n, k)
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", open(o).read())]
    PH, PW = ssim_lib.BWD_TILE_H, ssim_lib.BWD_TILE_W
    assert len(lds) == 3 and max(lds) <= 32768
    assert sorted(lds)[-1] == 2 * (PH + 12) * (PW + 12) * 4 + 3 * (PH + 6) * (PW + 6) * 8
    assert sorted(lds)[-2] == 2 * (ssim_lib.TILE_H + 6) * 72 * 4 + 32
