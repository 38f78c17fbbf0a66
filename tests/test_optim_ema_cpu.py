"""The weight EMA of the fused optimizer step without a GPU: the float32 restatement the GPU tests compare bit for bit
(tests/optim_ema_ref.py) against a float64 EMA within the bar derived in that file, and against torch's own
AveragedModel + get_ema_multi_avg_fn; the decay schedule; the layout of bmc_adam_ema_t and the companion header
include/bmc_hip_ema.h against the library's ABI text and the binding; the refusals of bmc_hip.optim.Adam(ema_decay=, ema_warmup=)
that need no device; an "ema" key through torch.optim.Adam's state dict; the device assembly of csrc/optim_ema.hip."""
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
import optim_asm
import optim_ema_ref as E

SCALES = (1e-8, 1e-4, 1.0, 1e3)


def _walk(rng, n, scale):
    """A random walk of float32 weights: steps of a hundredth of the scale, as an optimizer moves them."""
    p = (rng.standard_normal(n) * scale).astype(np.float32)
    while True:
        yield p
        p = (p + (rng.standard_normal(n) * scale * 1e-2).astype(np.float32)).astype(np.float32)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("warmup", [False, True], ids=["flat", "warmup"])
@pytest.mark.parametrize("decay", [0.0, 0.5, 0.999, 0.9999])
def test_float32_restatement_stays_within_the_derived_bar_of_float64(decay, warmup):
    """200 updates of random walks at the four scales; the worst ratio error / bar is printed, it must not exceed 1."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for scale in SCALES:
        walk = _walk(rng, 257, scale)
        p0 = next(walk)
        e32, ref = p0.copy(), E.Ema64(p0)
        for t in range(1, 201):
            p = next(walk)
            e32 = E.ema32(e32, p, E.weight32(decay, warmup, t))
            e64 = ref.update(p, decay, warmup, t)
            err = np.abs(e32.astype(np.float64) - e64)
            assert (err <= ref.bar).all(), (scale, t, float((err / ref.bar).max()))
            worst = max(worst, float((err / ref.bar).max()))
        assert ref.updates == 200
    print("decay %g warmup %d: worst error / bar %.3f" % (decay, warmup, worst))
    assert worst <= 1.0


def test_decay_zero_gives_the_weights_themselves_when_the_difference_is_exact():
    """w = 1: e' = e + (p - e).  For p and e within a factor of two of each other the difference is exact (Sterbenz) and e' == p."""
    rng = np.random.default_rng(12)
    e = (1.0 + rng.random(1000)).astype(np.float32)
    p = (e * (1.0 + 0.4 * rng.random(1000))).astype(np.float32)
    assert E.weight32(0.0, False, 5) == np.float32(1.0) and np.array_equal(E.ema32(e, p, np.float32(1.0)), p)


@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_restatement_agrees_with_torch_averaged_model(decay):
    """torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)) on the CPU in float32: its first update copies
    the weights, every later one is lerp(ema, p, 1 - decay).  Both stay within the bar of the float64 EMA started from that copy."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    rng = np.random.default_rng(13)
    for scale in SCALES:
        walk = _walk(rng, 129, scale)
        model = torch.nn.Module()
        model.w = torch.nn.Parameter(torch.from_numpy(next(walk).copy()))
        avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))
        avg.update_parameters(model)                         # n_averaged == 0: a copy
        e32, ref = model.w.detach().numpy().copy(), E.Ema64(model.w.detach().numpy())
        assert np.array_equal(avg.module.w.detach().numpy(), e32)
        for t in range(1, 101):
            p = next(walk)
            with torch.no_grad():
                model.w.copy_(torch.from_numpy(p))
            avg.update_parameters(model)
            e32 = E.ema32(e32, p, E.weight32(decay, False, t))
            ref.update(p, decay, False, t)
            theirs = avg.module.w.detach().numpy().astype(np.float64)
            assert (np.abs(theirs - ref.e) <= ref.bar).all() and (np.abs(e32 - ref.e) <= ref.bar).all(), (scale, t)


# ------------------------------------------------------------------ the schedule
def test_decay_schedule():
    from bmc_hip import optim
    assert E.decay_at(0.999, True, 1) == 0.1 == optim.ema_decay_at(0.999, True, 1) and E.decay_at(0.999, False, 1) == 0.999
    assert E.decay_at(0.05, True, 1) == 0.05                 # a decay below the ramp's start is never raised
    for decay in (0.5, 0.9, 0.999, 0.9999):
        seq = [float(E.decay_at(decay, True, t)) for t in range(1, 100002)]
        assert all(b >= a for a, b in zip(seq, seq[1:])) and max(seq) == decay
        first = next(t for t in range(1, 100002) if t / (t + 9.0) >= decay)
        assert seq[first - 1] == decay and seq[first - 2] < decay and seq[first - 2] == (first - 1) / (first + 8.0)
    assert next(t for t in range(1, 100) if t / (t + 9.0) >= 0.5) == 9
    for decay, warmup, t in ((0.999, True, 1), (0.999, True, 37), (0.9999, True, 99999), (0.5, False, 3), (0.0, False, 1), (0.0, True, 4)):
        w = E.weight32(decay, warmup, t)
        assert type(w) is np.float32 and float(w) == optim.ema_weight(decay, warmup, t)
        assert float(w) == float(np.float32(1.0 - float(E.decay_at(decay, warmup, t))))
    assert optim.ema_weight(0.0, False, 1) == 1.0 and optim.ema_weight(0.999, True, 1) == float(np.float32(0.9))


# ------------------------------------------------------------------ struct, header, exports
def test_companion_header_matches_its_abi_text_and_binding():
    """include/bmc_hip_ema.h by the header's text (abi_ref's regular expressions and classes) and by a C compile of it, against
    bmc_ema_abi() and what bmc_hip/ema_lib.py installs.  bmc_hip.h's own tables do not grow: lib.EXPORTS is what it was."""
    from bmc_hip import ema_lib, lib
    from bmc_hip.optim import CHUNK_DTYPE
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(abi_ref.INCLUDE, "bmc_hip_ema.h")).read(), flags=re.S)
    declared = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?[a-z][a-z ]*\*?)\s*\b(bmc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, re.M):
        params = [p.strip() for p in params.split(",")]
        declared[name] = [abi_ref.classify(ret)] + ([] if params == ["void"] else [abi_ref.classify(p) for p in params])
    entry = ["bmc_adam_ema_step", "bmc_adam_ema_step_capturable", "bmc_adam_ema_step_clipped", "bmc_adam_ema_step_clipped_capturable"]
    assert sorted(declared) == sorted(ema_lib.FUNCTIONS) == sorted(entry + ["bmc_ema_abi", "bmc_ema_swap"])
    assert not set(declared) & set(lib.FUNCTIONS) and not set(ema_lib.STRUCTS) & set(lib.STRUCTS)
    assert set(lib.EXPORTS) == set(abi_ref.functions()) and len(lib.EXPORTS) == 76 and "bmc_adam_ema_t" not in lib.STRUCTS
    for name, kinds in declared.items():                     # the header's text against the compiler's description
        got = [c.replace("s:", "") if c.startswith("s:") else c.split(":")[0] for c in ema_lib.FUNCTIONS[name]]
        assert got == kinds, (name, got, kinds)
        assert lib.has_symbol(name)
    # each twin is its original with the struct added after the hyper-parameters
    for name, orig in zip(entry, ("bmc_adam_step", "bmc_adam_step_capturable", "bmc_adam_step_clipped", "bmc_adam_step_clipped_capturable")):
        want = list(lib.FUNCTIONS[orig])
        want.insert(4, "s:bmc_adam_ema_t")
        assert ema_lib.FUNCTIONS[name] == want, name
    assert ema_lib._adam_ema_step.argtypes[3] is ema_lib.AdamEma and ema_lib._adam_ema_step_clip.argtypes[4] is lib.AdamClip
    assert ema_lib.FUNCTIONS["bmc_ema_swap"] == ["i4", "p:bmc_adam_chunk_t", "p", "i4", "p"]
    assert re.findall(r"^\}\s*(bmc_[a-z0-9_]+_t)\s*;", text, re.M) == list(ema_lib.STRUCTS) == ["bmc_adam_ema_t"]
    assert re.findall(r"^#define[ \t]+(BMC_[A-Z0-9_]+)[ \t]+\S", text, re.M) == []
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no host C compiler"
    fields = ["e", "decay", "w", "warmup"]
    body = ['printf("%d\\n", (int)sizeof(bmc_adam_ema_t));', 'printf("%d %d\\n", (int)sizeof(bmc_adam_chunk_t), (int)sizeof(bmc_adam_hyper_t));']
    body += ['printf("%%d %%d\\n", (int)offsetof(bmc_adam_ema_t, %s), (int)sizeof(((bmc_adam_ema_t*)0)->%s));' % (f, f) for f in fields]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "bmc_hip_ema.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(body)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run([cc, "-I" + abi_ref.INCLUDE, os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    st = ema_lib.STRUCTS["bmc_adam_ema_t"]
    assert out[0] == st.size == C.sizeof(ema_lib.AdamEma) == 24 and st.align == 8 and list(st.fields) == fields
    assert out[1:3] == [48, 64] == [CHUNK_DTYPE.itemsize, C.sizeof(lib.AdamHyper)]          # the pinned structs stay
    for f, off, size in zip(fields, out[3::2], out[4::2]):
        assert (st.fields[f].offset, st.fields[f].size) == (off, size) == (getattr(ema_lib.AdamEma, f).offset, getattr(ema_lib.AdamEma, f).size)
    kinds = dict(ema_lib.AdamEma._fields_)
    assert [kinds[f] for f in fields] == [C.c_void_p, C.c_double, C.c_float, C.c_int]


def test_ema_chunk_table():
    """The EMA pointer of a chunk is the average's address plus the chunk's byte offset; an average that is not 16-byte aligned
    clears `aligned` for its chunks only; chunk_table itself gives what it gave."""
    from bmc_hip.optim import CHUNK, chunk_table, ema_chunk_table
    a = [1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20]
    rows = [(*a, 2 * CHUNK + 1, 6 << 20), (*[v + (1 << 19) for v in a], 7, (7 << 20) + 4), (a[0], None, a[2], a[3], a[4], 99, 8 << 20),
            (*[v + (1 << 18) for v in a[:4]], None, 5, 9 << 20)]
    tab, e = ema_chunk_table(rows)
    assert np.array_equal(tab[["p", "g", "m", "v", "vmax", "n"]], chunk_table([r[:6] for r in rows])[["p", "g", "m", "v", "vmax", "n"]])
    assert tab["n"].tolist() == [CHUNK, CHUNK, 1, 7, 5] and tab["aligned"].tolist() == [1, 1, 1, 0, 1]
    assert e.dtype == np.uint64 and e.tolist() == [6 << 20, (6 << 20) + 4 * CHUNK, (6 << 20) + 8 * CHUNK, (7 << 20) + 4, 9 << 20]
    tab, e = ema_chunk_table([(a[0] + 4, *a[1:], 9, 6 << 20)])                               # an unaligned parameter stays unaligned
    assert tab["aligned"].tolist() == [0] and e.tolist() == [6 << 20]
    tab, e = ema_chunk_table([])
    assert len(tab) == 0 and len(e) == 0


# ------------------------------------------------------------------ refusals without a device
def test_ema_refusals_without_a_device():
    """Bad values raise before the parameters are looked at: the CPU parameter here would otherwise be the error."""
    from bmc_hip.optim import Adam
    w = lambda: [torch.nn.Parameter(torch.zeros(3, 2))]
    for bad in (1, 1.0, -0.1, 1.5, float("nan"), float("inf"), True, False, torch.tensor(0.5), "0.9", np.nextafter(1.0, 2.0)):
        with pytest.raises(ValueError, match="ema_decay"):
            Adam(w(), ema_decay=bad)
    with pytest.raises(ValueError, match="ema_warmup=True needs ema_decay"):
        Adam(w(), ema_warmup=True)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="ema_warmup"):
            Adam(w(), ema_decay=0.9, ema_warmup=bad)
    for good in (dict(ema_decay=0), dict(ema_decay=0.0), dict(ema_decay=0.999, ema_warmup=True), dict(ema_decay=np.float32(0.5)),
                 dict(ema_decay=np.nextafter(1.0, 0.0)), dict(ema_decay=0.5, max_grad_norm=1.0, nonfinite="skip")):
        with pytest.raises(ValueError, match="is on cpu"):                 # accepted; the parameter is what is refused
            Adam(w(), **good)


def test_an_ema_key_travels_through_torch_adam_state_dicts():
    """A hand-built state dict with an "ema" entry per parameter loads into torch.optim.Adam on the CPU, survives a step there
    untouched and comes back out: what lets our checkpoints load into torch's optimizer."""
    torch.manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
    opt = torch.optim.Adam(params, lr=1e-3, amsgrad=True, foreach=False)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()
    sd = opt.state_dict()
    emas = [torch.randn(5), torch.randn(2, 3)]
    for i, e in enumerate(emas):
        sd["state"][i]["ema"] = e.clone()
    fresh = torch.optim.Adam(params, lr=1e-3, amsgrad=True, foreach=False)
    fresh.load_state_dict(sd)
    assert all(torch.equal(fresh.state[p]["ema"], e) for p, e in zip(params, emas))
    fresh.step()
    out = fresh.state_dict()
    assert all(torch.equal(out["state"][i]["ema"], e) for i, e in enumerate(emas))
    assert sorted(out["state"][0]) == ["ema", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "step"] and float(out["state"][0]["step"]) == 2.0


# ------------------------------------------------------------------ the device assembly
@pytest.mark.skipif(not os.path.exists(optim_asm.HIPCC), reason="hipcc not installed")
def test_device_assembly_of_the_ema_kernels():
    """csrc/optim_ema.hip compiled for gfx950 as tests/optim_asm.py compiles csrc/optim.hip; nothing is executed.  13 kernels: eight
    unclipped and four clipped step kernels and the exchange.  None has a flat_ memory instruction, an atomic or scratch memory; the
    step kernels hold the 16-byte loads and stores of the aligned path, one stream more than their originals; no kernel runs at
    fewer than 3 waves per SIMD (a full chunk's 24 loads cost the amsgrad kernels one wave against their originals' 4: DESIGN.md 7)."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "optim_ema.s")
        r = subprocess.run([optim_asm.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(optim_asm.ROOT, "include"),
                            "-S", "--cuda-device-only", "-o", out, os.path.join(optim_asm.CSRC, "optim_ema.hip")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        found, cur = {}, None
        for ln in open(out):
            m = re.match(r"^(_Z\w+):", ln)
            if m:
                cur = found[m.group(1)] = {"bad": 0, "ld16": 0, "st16": 0}
                continue
            if cur is None:
                continue
            code = ln.split(";")[0]
            cur["bad"] += bool(re.search(r"\bflat_(load|store|atomic)|\bglobal_atomic|\bscratch_", code))
            cur["ld16"] += "global_load_dwordx4" in code
            cur["st16"] += "global_store_dwordx4" in code
            m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)", ln)
            if m:
                cur[m.group(1)] = int(m.group(2))
                if m.group(1) == "Occupancy":
                    cur = None
    count = lambda part: sum(part in n for n in found)
    assert (count("adam_ema_kernel"), count("clip_step_ema_kernel"), count("ema_swap_kernel"), len(found)) == (8, 4, 1, 13), sorted(found)
    for n, k in sorted(found.items()):
        print(n, k)
        assert k["bad"] == 0 and k["ScratchSize"] == 0 and k["Occupancy"] >= 3, (n, k)
        if "swap" in n:
            assert k["ld16"] >= 2 and k["st16"] >= 2, (n, k)
        else:
            assert k["ld16"] >= 5 and k["st16"] >= 4, (n, k)
