"""The clipped optimizer step without a GPU: the float64 restatement the GPU tests measure against (tests/optim_clip_ref.py) is
checked against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64; the float32 coefficient function against its
float64 value; the layout of bmc_adam_clip_t, the exported symbols, the refusals of bmc_hip.optim.Adam(max_grad_norm=, nonfinite=)
that need no device; and the device assembly of the clipped kernels of csrc/optim.hip."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import optim_asm
import optim_clip_ref as CR
import optim_ref as R

ROOT = optim_asm.ROOT


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("setting", R.SETTINGS, ids=lambda s: "amsgrad%d_wd%g" % (s["amsgrad"], s["weight_decay"]))
def test_restatement_equals_clip_grad_norm_and_torch_adam_in_float64(setting):
    """Five steps; the gradients grow from step to step, so that max_norm = 4 clips steps 3..5 and not steps 1..2.  1e-12 relative:
    the two differ in how the norm is added up and in torch's reciprocal-and-multiply against a division."""
    cfg = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, **setting)
    max_norm = 4.0
    g = torch.Generator().manual_seed(5)
    params = [torch.randn(37, generator=g, dtype=torch.float64), torch.randn(4, 9, generator=g, dtype=torch.float64)]
    tp = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.Adam(tp, foreach=False, **cfg)
    ref = CR.ClippedAdam64(params, max_norm, **cfg)
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    clipped = []
    for step in range(5):
        # float32 values (the restatement's norm takes float32 gradients), held in float64 tensors for torch
        grads = [(torch.randn(p.shape, generator=g) * s * 2.0 ** step).double() for p, s in zip(params, (0.25, 1e-4))]
        for p, gr in zip(tp, grads):
            p.grad = gr.clone()
        total = torch.nn.utils.clip_grad_norm_(tp, max_norm, foreach=False)
        opt.step()
        ref.step([gr.numpy() for gr in grads])
        assert abs(ref.last[0] - float(total)) <= 1e-14 * float(total)
        clipped.append(ref.last[1] < 1.0)
        for i, p in enumerate(tp):
            st = opt.state[p]
            assert rel(ref.p[i], p.detach()) <= 1e-12
            assert rel(ref.m[i], st["exp_avg"]) <= 1e-12 and rel(ref.v[i], st["exp_avg_sq"]) <= 1e-12
            if setting["amsgrad"]:
                assert rel(ref.vmax[i], st["max_exp_avg_sq"]) <= 1e-12
    assert clipped == [False, False, True, True, True]


# ------------------------------------------------------------------ the float32 coefficient
def test_coefficient_special_cases():
    f = np.float32
    assert CR.coeff32(0.0, 1.0) == f(1.0) and CR.coeff32(0.0, 1e-3) == f(1.0)          # 1e-3 / 1e-6 clamps
    c = CR.coeff32(2.5, 2.5)
    assert f(1.0) - f(1e-6) <= c < f(1.0)                                                # the 1e-6 of the denominator
    assert CR.coeff32(float("inf"), 1.0) == 0.0 and np.isnan(CR.coeff32(float("nan"), 1.0))
    assert CR.coeff32(3.0, float("inf")) == f(1.0) and CR.coeff32(1e300, 1.0) == 0.0     # never clip; a norm beyond float32
    assert np.isnan(CR.coeff32(float("inf"), float("inf")))                              # Inf / Inf
    assert all(isinstance(CR.coeff32(n, 1.0), np.float32) for n in (0.0, 2.0, float("inf"), float("nan")))
    assert CR.coeff64(0.0, 1.0) == 1.0 and CR.coeff64(float("inf"), 1.0) == 0.0 and np.isnan(CR.coeff64(float("nan"), 1.0))


def test_coefficient_is_three_float32_roundings_from_float64():
    """2 000 random gradient sets (one scale of 1e-8, 1e-4, 1, 1e3 per tensor), max_norm between a third and three times the norm:
    |c32 - c64| <= 3 * 2^-24 * c64 (the rounding of the norm, of the sum, of the quotient)."""
    rng = np.random.default_rng(7)
    worst, clipped = 0.0, 0
    for _ in range(2000):
        k = int(rng.integers(1, 5))
        grads = [(rng.standard_normal(int(rng.integers(1, 40))) * (1e-8, 1e-4, 1.0, 1e3)[int(rng.integers(0, 4))]).astype(np.float32)
                 for _ in range(k)]
        norm = CR.global_norm64(grads)
        max_norm = float(np.float32(norm * rng.uniform(1 / 3, 3)))
        if not max_norm > 0:
            continue
        c32, c64 = CR.coeff32(norm, max_norm), CR.coeff64(norm, max_norm)
        clipped += c64 < 1.0
        worst = max(worst, abs(float(c32) - float(c64)) / float(c64))
    print("worst relative distance %.3e over 2000 sets, %d clipped" % (worst, clipped))
    assert worst <= 3 * 2.0 ** -24 and 500 < clipped < 1500


def test_global_norm_is_exact():
    rng = np.random.default_rng(9)
    grads = [(rng.standard_normal(n) * s).astype(np.float32) for n, s in ((5, 1e-8), (4097, 1.0), (300, 1e3))] + [None]
    want = float(np.sqrt(sum(np.sum(g.astype(np.longdouble) ** 2) for g in grads[:3])))
    assert abs(CR.global_norm64(grads) - want) <= np.spacing(want) and CR.global_norm64([None]) == 0.0      # one float64 ulp


# ------------------------------------------------------------------ struct, exports, refusals
def test_clip_struct_layout_matches_a_c_compile_of_the_header():
    import abi_ref
    from bmc_hip import lib
    from bmc_hip.optim import CHUNK_DTYPE
    fields = [f[0] for f in lib.AdamClip._fields_]
    assert sorted(fields) == sorted(["partial_sq", "n_partials", "max_norm", "skip_nonfinite", "info", "skipped"])
    structs = abi_ref.compiled_header()[0]
    size, compiled = structs["bmc_adam_clip_t"]
    assert [structs["bmc_adam_chunk_t"][0], structs["bmc_adam_hyper_t"][0]] == [48, 64] == [CHUNK_DTYPE.itemsize, C.sizeof(lib.AdamHyper)]
    assert size == C.sizeof(lib.AdamClip) and list(compiled) == fields
    assert [compiled[f][0] for f in fields] == [getattr(lib.AdamClip, f).offset for f in fields]
    assert [compiled[f][1] for f in fields] == [getattr(lib.AdamClip, f).size for f in fields]
    kinds = dict(lib.AdamClip._fields_)
    assert kinds["max_norm"] is C.c_float and kinds["n_partials"] is C.c_int and kinds["skip_nonfinite"] is C.c_int


def test_the_three_entry_points_are_exported():
    from bmc_hip import lib
    so = C.CDLL(lib.LIB_PATH)
    for name in ("bmc_adam_grad_sq", "bmc_adam_step_clipped", "bmc_adam_step_clipped_capturable"):
        assert name in lib.EXPORTS and lib.has_symbol(name) and hasattr(so, name)
    assert lib._adam_step_clip.argtypes[3] is lib.AdamClip and lib._adam_step_clip_cap.argtypes[4] is lib.AdamClip


def test_clip_refusals_without_a_device():
    """Bad values raise before the parameters are looked at: the CPU parameter here would otherwise be the error."""
    from bmc_hip.optim import Adam
    w = lambda: [torch.nn.Parameter(torch.zeros(3, 2))]
    for bad in (0, 0.0, -1.0, float("nan"), True, False, torch.tensor(1.0), "1", 1e-60):
        with pytest.raises(ValueError, match="max_grad_norm"):
            Adam(w(), max_grad_norm=bad)
    for bad in ("ignore", None, True, "Skip"):
        with pytest.raises(ValueError, match="nonfinite"):
            Adam(w(), nonfinite=bad)
    for good in (dict(max_grad_norm=1.0), dict(max_grad_norm=3), dict(nonfinite="skip"), dict(max_grad_norm=float("inf")),
                 dict(max_grad_norm=np.float32(0.5), nonfinite="skip")):
        with pytest.raises(ValueError, match="is on cpu"):                 # accepted; the parameter is what is refused
            Adam(w(), **good)
    with pytest.raises(ValueError, match="decoupled_weight_decay"):        # AdamW stays out
        Adam(w(), max_grad_norm=1.0, decoupled_weight_decay=True)


# ------------------------------------------------------------------ the device assembly
@pytest.mark.skipif(not os.path.exists(optim_asm.HIPCC), reason="hipcc not installed")
def test_device_assembly_of_the_clipped_step():
    """csrc/optim.hip, the file tests/test_optim_cpu.py reads and with its assertions on every kernel (tests/optim_asm.py); nothing
    is executed.  The four clipped step kernels keep the 16-byte loads and stores of the aligned path; the norm kernel has 16-byte
    loads and no 16-byte store."""
    steps, norms = optim_asm.check_family("clip_step_kernel"), optim_asm.check_family("grad_sq_kernel")
    assert len(steps) == 4 and len(norms) == 1
    for n, k in steps.items():
        assert k["ld16"] >= 4 and k["st16"] >= 3, (n, k)
    for n, k in norms.items():
        assert k["ld16"] >= 1 and k["st16"] == 0, (n, k)
