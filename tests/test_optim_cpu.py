"""The optimizer step without a GPU: the float64 restatement the GPU tests measure against (tests/optim_ref.py) is checked
against the golden reference trajectory, the oracle and torch.optim.Adam in float64; the chunk-table builder, the struct layouts,
the exported symbols and the refusals of bmc_hip.optim.Adam that need no device; and the device assembly of csrc/optim.hip."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import optim_asm
import optim_ref as R

ROOT = optim_asm.ROOT


# ------------------------------------------------------------------ the restatement
def test_restatement_reproduces_the_golden_trajectory_and_the_oracle():
    """golden/adam.npz: three steps of the reference's optimizer on two tensors; 1e-7 absolute, the bar of
    tests/test_oracle_golden.py::test_adam_amsgrad.  The oracle's own float64 run is met to rounding."""
    from oracle import bmc_oracle as O
    z = R.golden()
    ref = R.Adam64([z["w0"], z["w1"]], **R.GOLDEN_CFG)
    ws = [torch.tensor(z["w0"]).double(), torch.tensor(z["w1"]).double()]
    st = {"step": 0, "m": [torch.zeros_like(w) for w in ws], "v": [torch.zeros_like(w) for w in ws], "vmax": [torch.zeros_like(w) for w in ws]}
    for step in range(3):
        grads = [z[f"g{step}_{i}"] for i in range(2)]
        ref.step(grads)
        O.adam_amsgrad_step(ws, [torch.tensor(g).double() for g in grads], st)
        for i in range(2):
            assert np.abs(ref.p[i].numpy() - z[f"w_after{step}_{i}"]).max() < 1e-7
            assert float((ref.p[i] - ws[i]).abs().max()) < 1e-15 * float(ws[i].abs().max())


@pytest.mark.parametrize("setting", R.SETTINGS, ids=lambda s: "amsgrad%d_wd%g" % (s["amsgrad"], s["weight_decay"]))
def test_restatement_equals_torch_adam_in_float64(setting):
    cfg = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, **setting)
    g = torch.Generator().manual_seed(5)
    params = [torch.randn(37, generator=g, dtype=torch.float64), torch.randn(4, 9, generator=g, dtype=torch.float64)]
    tp = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.Adam(tp, foreach=False, **cfg)
    ref = R.Adam64(params, **cfg)
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    for _ in range(4):
        grads = [torch.randn(p.shape, generator=g, dtype=torch.float64) * s for p, s in zip(params, (1.0, 1e-4))]
        for p, gr in zip(tp, grads):
            p.grad = gr.clone()
        opt.step()
        ref.step(grads)
        for i, p in enumerate(tp):
            st = opt.state[p]
            assert rel(ref.p[i], p.detach()) <= 1e-15
            assert rel(ref.m[i], st["exp_avg"]) <= 1e-15 and rel(ref.v[i], st["exp_avg_sq"]) <= 1e-15
            if setting["amsgrad"]:
                assert rel(ref.vmax[i], st["max_exp_avg_sq"]) <= 1e-15


# ------------------------------------------------------------------ the chunk table
@pytest.mark.parametrize("n", [1, 3, 4095, 4096, 4097, 2 * 4096 + 5])
def test_chunk_table_sizes(n):
    from bmc_hip.optim import CHUNK, chunk_table
    base = [1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20]
    tab = chunk_table([(*base, n), (6 << 20, 7 << 20, 8 << 20, 9 << 20, 0, 7)])
    k = (n + CHUNK - 1) // CHUNK
    assert len(tab) == k + 1 and tab["n"][:k].sum() == n and tab["n"].max() <= CHUNK and tab["n"].min() >= 1
    assert tab["n"][:k - 1].tolist() == [CHUNK] * (k - 1) and tab["n"][k - 1] == n - (k - 1) * CHUNK
    for c, key in enumerate(("p", "g", "m", "v", "vmax")):
        assert tab[key][:k].tolist() == [base[c] + 4 * CHUNK * j for j in range(k)]       # no chunk spans two tensors
    assert tab["aligned"].tolist() == [1] * (k + 1)
    assert (tab["p"][k], tab["vmax"][k], tab["n"][k]) == (6 << 20, 0, 7)                   # no amsgrad: NULL stays NULL


def test_chunk_table_alignment_flag_and_skipped_parameters():
    from bmc_hip.optim import chunk_table
    a = [1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20]
    for which in range(5):
        for off in (1, 2, 3):                         # an odd (or any non-multiple-of-4) element offset of ONE of the five tensors
            b = list(a)
            b[which] += 4 * off
            tab = chunk_table([(*b, 5000), (*a, 5000)])
            assert tab["aligned"].tolist() == [0, 0, 1, 1]
    assert chunk_table([(*[v + 16 for v in a], 9)])["aligned"].tolist() == [1]
    tab = chunk_table([(*a, 10), (a[0], None, a[2], a[3], a[4], 99999), (a[0] + 64, a[1], a[2], a[3], None, 3)])
    assert tab["n"].tolist() == [10, 3] and tab["p"].tolist() == [a[0], a[0] + 64]     # grad is None: left out
    assert len(chunk_table([])) == 0 and len(chunk_table([(1, None, 2, 3, 4, 5)])) == 0


def test_struct_layouts_match_a_c_compile_of_the_header():
    import abi_ref
    from bmc_hip import lib
    from bmc_hip.optim import CHUNK, CHUNK_DTYPE
    chunk = ["p", "g", "m", "v", "vmax", "n", "aligned"]
    hyper = [f[0] for f in lib.AdamHyper._fields_]
    structs, constants = abi_ref.compiled_header()
    (chunk_size, c_chunk), (hyper_size, c_hyper) = structs["bmc_adam_chunk_t"], structs["bmc_adam_hyper_t"]
    assert [chunk_size, hyper_size, constants["BMC_ADAM_CHUNK"]] == [CHUNK_DTYPE.itemsize, C.sizeof(lib.AdamHyper), CHUNK]
    assert [c_chunk[f][0] for f in chunk] == [CHUNK_DTYPE.fields[f][1] for f in chunk]
    assert list(c_hyper) == hyper and [c_hyper[f][0] for f in hyper] == [getattr(lib.AdamHyper, f).offset for f in hyper]
    assert [CHUNK_DTYPE.fields[f][0].itemsize for f in chunk] == [8] * 5 + [4, 4]


def test_both_entry_points_are_exported():
    from bmc_hip import lib
    so = C.CDLL(lib.LIB_PATH)
    for name in ("bmc_adam_step", "bmc_adam_step_capturable"):
        assert name in lib.EXPORTS and lib.has_symbol(name) and hasattr(so, name)


def test_step_hyper_rounds_torchs_float64_values_once():
    from bmc_hip.optim import step_hyper
    h = step_hyper(1e-4, 0.9, 0.999, 1e-8, 1e-5, True, 7.0)
    f = lambda v: float(np.float32(v))
    assert h.step_size == f(1e-4 / (1 - 0.9 ** 7.0)) and h.bias_correction2_sqrt == f((1 - 0.999 ** 7.0) ** 0.5)
    assert (h.beta1, h.one_minus_beta1, h.beta2, h.one_minus_beta2) == (f(0.9), f(1 - 0.9), f(0.999), f(1 - 0.999))
    assert (h.eps, h.weight_decay, h.amsgrad, h.lr, h.beta1_f64, h.beta2_f64) == (f(1e-8), f(1e-5), 1, 1e-4, 0.9, 0.999)


# ------------------------------------------------------------------ refusals that need no device
def test_refusals_without_a_device():
    from bmc_hip.optim import Adam
    w = lambda **kw: [torch.nn.Parameter(torch.zeros(3, 2, **kw))]
    with pytest.raises(ValueError, match=r"#0 of group 0 \(shape \(3, 2\)\) is on cpu"):
        Adam(w())
    with pytest.raises(ValueError, match="'fc.weight'"):
        Adam([("fc.weight", w()[0])])
    for flag in ("maximize", "foreach", "fused", "differentiable", "decoupled_weight_decay"):
        with pytest.raises(ValueError, match=flag):
            Adam(w(), **{flag: True})
    with pytest.raises(ValueError, match="tensor lr"):
        Adam(w(), lr=torch.tensor(1e-3))
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            Adam(w(), **bad)
    assert issubclass(Adam, torch.optim.Optimizer) and Adam.__name__ == "Adam"


# ------------------------------------------------------------------ the device assembly
@pytest.mark.skipif(not os.path.exists(optim_asm.HIPCC), reason="hipcc not installed")
def test_device_assembly_of_the_step():
    """csrc/optim.hip compiled and read by tests/optim_asm.py; nothing is executed.  Every kernel of the file (14, one advance
    kernel among them): no flat_ memory instruction (table pointers are read through address-space(1) accessors), no scratch
    memory, no fewer waves per SIMD than before the shared walk; the eight step kernels (amsgrad x norm x capturable) hold the
    16-byte loads and stores of the aligned path."""
    steps = optim_asm.check_family("adam_kernel")
    assert len(steps) == 8
    for n, k in steps.items():
        assert k["ld16"] >= 4 and k["st16"] >= 3, (n, k)
