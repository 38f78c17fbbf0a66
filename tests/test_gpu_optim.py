"""bmc_hip.optim.Adam on the MI355X (csrc/optim.hip, include/bmc_hip.h "optimizer step").

The yardstick throughout is torch.optim.Adam(foreach=False) in fp32 on the same GPU, fed identical gradients; both are measured
against the float64 restatement of tests/optim_ref.py (itself pinned by tests/test_optim_cpu.py).  Per tensor and step
    e(x) = max|x - x64| / max|x64|   for exp_avg, exp_avg_sq, max_exp_avg_sq          e(p) = max|p - p64| / lr
and the HIP optimizer passes when  e_hip <= 2 * e_torch + 1e-7  for every tensor and every step (the factor 2: its rounding points
are the six of the header, not ATen's lerp_ / addcmul_ / addcdiv_).  Gradients have ONE scale per tensor (1e-8, 1e-4, 1, 1e3 across
tensors).  On top of that the kernel is compared BIT FOR BIT with a numpy float32 evaluation of the six lines, one rounding each.

Measured (MI355X, this file; the largest value over tensors and steps of each test, printed by the run with -s):
  (e_hip / e_torch)                  p                    exp_avg              exp_avg_sq           max_exp_avg_sq
  sizes, wd 0 (amsgrad on and off)   5.53e-03 / 5.53e-03  1.35e-07 / 1.35e-07  1.96e-07 / 1.54e-07  1.96e-07 / 1.54e-07
  sizes, wd 1e-5 (amsgrad on / off)  5.53e-03 / 5.53e-03  1.29e-07 / 5.01e-08  2.31e-07 / 1.38e-07  2.31e-07 / 1.38e-07
  zero gradients, wd 1e-5            3.53e-04 / 3.53e-04  6.42e-08 / 6.42e-08  1.76e-07 / 7.05e-08  1.76e-07 / 7.05e-08
  grad is None                       3.92e-04 / 3.92e-04  8.30e-08 / 3.78e-08  2.00e-07 / 1.11e-07  2.00e-07 / 1.11e-07
  interchange, torch first           5.02e-04 / 5.02e-04  1.53e-07 / 9.61e-08  1.77e-07 / 1.77e-07  1.77e-07 / 1.77e-07
  interchange, hip first             5.02e-04 / 5.02e-04  9.61e-08 / 9.61e-08  1.77e-07 / 1.77e-07  1.77e-07 / 1.77e-07
  StepLR                             1.26e-04 / 1.26e-04  9.54e-08 / 7.50e-08  1.91e-07 / 1.91e-07  1.58e-07 / 1.34e-07
  GradAllReducer                     2.63e-05 / 2.63e-05  7.63e-08 / 4.14e-08  1.77e-07 / 8.25e-08  1.77e-07 / 8.25e-08
  capturable (five steps)            4.17e-04 / 4.17e-04  1.12e-07 / 1.12e-07  1.99e-07 / 2.55e-07  1.99e-07 / 2.55e-07
The aligned and the packed layout give the same figures (the two load paths are bit-identical), and every step of the size cases
equals the numpy float32 evaluation bit for bit.  e(p) is the rounding of p itself (half an ulp of |p| ~ 3 over lr = 1e-4), the
same for both optimizers.
"""
import numpy as np
import pytest
import torch

import optim_ref as R
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 4096                        # floats of NaN before and after every guarded tensor
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 12293]
SCALES = [1e-8, 1e-4, 1.0, 1e3]
KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")
WORST = {}                          # test -> {quantity: (e_hip, e_torch)}: the table above


@pytest.fixture(scope="module", autouse=True)
def _print_measured():
    yield
    for name, row in WORST.items():
        print("\n%-34s " % name + "  ".join("%s %.2e / %.2e" % (k, a, b) for k, (a, b) in sorted(row.items())), end="")
    print()


def _setting_id(s):
    return "amsgrad%d_wd%g" % (s["amsgrad"], s["weight_decay"])


def _guarded(dev, sizes, aligned):
    """Views of ONE buffer, every tensor between NaN guards of GUARD floats.  aligned: every tensor starts at a multiple of four
    elements (16 bytes); otherwise they are packed, so that most start at an odd element offset."""
    offs, at = [], 0
    for n in sizes:
        at += GUARD
        if aligned:
            at = (at + 3) // 4 * 4
        offs.append(at)
        at += n
    buf = torch.full((at + GUARD,), float("nan"), device=dev)
    mask = torch.ones(at + GUARD, dtype=torch.bool, device=dev)
    views = []
    for n, o in zip(sizes, offs):
        views.append(buf[o:o + n])
        mask[o:o + n] = False
    return buf, mask, views


class Pair:
    """The HIP optimizer, the yardstick and the float64 restatement on copies of the same tensors."""

    def __init__(self, name, hip_params, cfg, hip_kwargs=None):
        from bmc_hip.optim import Adam
        self.name, self.cfg, self.lr = name, cfg, cfg["lr"]
        self.hp = hip_params
        self.tp = [torch.nn.Parameter(p.detach().clone()) for p in hip_params]
        self.hip = Adam(self.hp, **cfg, **(hip_kwargs or {}))
        self.torch = torch.optim.Adam(self.tp, foreach=False, **cfg)
        self.ref = R.Adam64([p.detach().cpu().numpy() for p in hip_params], **cfg)

    def feed(self, grads):
        for ps in (self.hp, self.tp):
            for p, g in zip(ps, grads):
                p.grad = None if g is None else g.detach().clone().view_as(p)

    def step(self, grads, **ref_override):
        self.feed(grads)
        self.hip.step()
        self.torch.step()
        self.ref.step([None if g is None else g.detach().cpu().numpy() for g in grads], **ref_override)

    def check(self, lr=None):
        """The bar, for every tensor that has state."""
        row = WORST.setdefault(self.name, {})
        for i, (ph, pt) in enumerate(zip(self.hp, self.tp)):
            if self.ref.steps[i] == 0:
                continue
            pairs = [("p", R.e_param(ph, self.ref.p[i], lr or self.lr), R.e_param(pt, self.ref.p[i], lr or self.lr))]
            sh, stt = self.hip.state[ph], self.torch.state[pt]
            for key, x64 in zip(KEYS, (self.ref.m[i], self.ref.v[i], self.ref.vmax[i])):
                if key in stt:
                    pairs.append((key, R.e_state(sh[key], x64), R.e_state(stt[key], x64)))
            for key, eh, et in pairs:
                if eh >= row.get(key, (-1.0, 0.0))[0]:
                    row[key] = (eh, et)
                assert eh <= 2 * et + 1e-7, (self.name, "tensor %d" % i, key, "e_hip %.3e" % eh, "e_torch %.3e" % et)


def _grads(gen, params, scales=SCALES):
    return [(torch.randn(p.shape, generator=gen) * scales[i % len(scales)]).to(p.device) for i, p in enumerate(params)]


def _params(dev, sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=gen).to(dev)) for n in sizes], gen


def _f32_step(p, g, m, v, vmax, step, lr, betas, eps, weight_decay, amsgrad):
    """The six lines on numpy float32 arrays: every operation rounded to float32 once (numpy's float32 add, multiply, divide and
    sqrt are IEEE), the hyper-parameters rounded as bmc_hip.optim.step_hyper rounds them."""
    f = np.float32
    omb1, beta2, omb2 = f(1 - betas[0]), f(betas[1]), f(1 - betas[1])
    step_size, bc2s = f(lr / (1 - betas[0] ** step)), f((1 - betas[1] ** step) ** 0.5)
    with np.errstate(all="ignore"):
        if weight_decay != 0:
            g = g + f(weight_decay) * p
        m = m + omb1 * (g - m)
        v = v * beta2 + omb2 * (g * g)
        if amsgrad:
            vmax = np.where(np.isnan(v) | np.isnan(vmax), f("nan"), np.maximum(vmax, v))
        den = np.sqrt(vmax if amsgrad else v) / bc2s + f(eps)
        p = p - step_size * (m / den)
    assert all(a.dtype == np.float32 for a in (p, m, v, vmax))
    return p, m, v, vmax


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1. the golden trajectory
def test_golden_trajectory():
    """tests/golden/adam.npz through the HIP optimizer: 15 and 7 elements, three steps, 1e-7 absolute against w_after*."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    z = R.golden()
    ws = [torch.nn.Parameter(torch.tensor(z[k]).to(dev)) for k in ("w0", "w1")]
    opt = Adam(ws, **R.GOLDEN_CFG)
    for step in range(3):
        for i, w in enumerate(ws):
            w.grad = torch.tensor(z[f"g{step}_{i}"]).to(dev)
        opt.step()
        for i, w in enumerate(ws):
            assert np.abs(w.detach().cpu().numpy() - z[f"w_after{step}_{i}"]).max() < 1e-7
    assert [float(opt.state[w]["step"]) for w in ws] == [3.0, 3.0] and all(not opt.state[w]["step"].is_cuda for w in ws)


# ------------------------------------------------------------------ 2. sizes, between guards
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "packed"])
@pytest.mark.parametrize("setting", R.SETTINGS, ids=_setting_id)
def test_sizes_between_guards(setting, aligned):
    """1 .. 12293 elements in one group, six steps, ONE launch per step; parameters and every state tensor are views of guarded
    buffers (packed: at odd element offsets -- the one-by-one path; aligned: the 16-byte path and its one-by-one tail).  Besides
    the bar against torch: bit for bit the float32 evaluation of the header's six lines."""
    dev = _gpu()
    from bmc_hip import optim
    cfg = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, **setting)
    gen = torch.Generator().manual_seed(11)
    bufs = [_guarded(dev, SIZES, aligned) for _ in range(4)]
    for _, _, views in bufs[1:]:
        for t in views:
            t.zero_()
    params = []
    for t in bufs[0][2]:
        t.copy_(torch.randn(t.shape, generator=gen))
        params.append(torch.nn.Parameter(t))
    assert all(p.data_ptr() == t.data_ptr() for p, t in zip(params, bufs[0][2]))
    assert aligned == all(p.data_ptr() % 16 == 0 for p in params)
    pair = Pair("sizes " + _setting_id(setting) + (" aligned" if aligned else " packed"), params, cfg)
    for i, p in enumerate(params):          # the state in guarded views too (what load_state_dict may hand the optimizer as well)
        st = dict(step=torch.tensor(0.0), exp_avg=bufs[1][2][i], exp_avg_sq=bufs[2][2][i])
        if setting["amsgrad"]:
            st["max_exp_avg_sq"] = bufs[3][2][i]
        pair.hip.state[p] = st
    f32 = [[p.detach().cpu().numpy()] + [np.zeros(p.numel(), np.float32) for _ in range(3)] for p in params]
    for step in range(6):
        grads = _grads(gen, params)
        n0 = optim.STEP_LAUNCHES
        pair.step(grads)
        assert optim.STEP_LAUNCHES == n0 + 1
        pair.check()
        for i, p in enumerate(params):
            f32[i] = list(_f32_step(f32[i][0], grads[i].cpu().numpy(), *f32[i][1:], step=step + 1.0, **cfg))
            st = pair.hip.state[p]
            got = [p, st["exp_avg"], st["exp_avg_sq"]] + ([st["max_exp_avg_sq"]] if setting["amsgrad"] else [])
            for name, a, b in zip(("p",) + KEYS, got, f32[i]):
                assert np.array_equal(a.detach().cpu().numpy().view(np.int32), b.view(np.int32)), (step, SIZES[i], name)
    torch.cuda.synchronize()
    for buf, mask, _ in bufs[:4 if setting["amsgrad"] else 3]:
        assert bool(torch.isnan(buf[mask]).all()), "a guard region was written"
    if not setting["amsgrad"]:
        assert all(bool((t == 0).all()) for t in bufs[3][2])


# ------------------------------------------------------------------ 3. unaligned gradients
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_gradients_that_are_views_of_a_flat_buffer(offset):
    """p.grad a view into a flat buffer at element offset 0..3 (GradAllReducer's buckets): bit-identical to the same steps with
    the gradients copied into fresh aligned tensors -- the one-by-one path and the 16-byte path round alike."""
    dev = _gpu()
    from bmc_hip.optim import Adam, chunk_table
    cfg = dict(lr=1e-3, weight_decay=1e-5, amsgrad=True)
    sizes = [5, 4097, 12293, 8]
    runs = []
    for flat_views in (True, False):
        params, gen = _params(dev, sizes, 23)
        opt = Adam(params, **cfg)
        for _ in range(2):
            grads = _grads(gen, params)
            if flat_views:
                flat = torch.zeros(offset + sum(sizes) + 3 * len(sizes), device=dev)
                at = offset
                for p, g in zip(params, grads):
                    view = flat[at:at + p.numel()]
                    view.copy_(g)
                    p.grad = view.view_as(p)
                    at += p.numel() + (-(p.numel()) % 4)         # every view keeps the element offset `offset` modulo 4
                assert all(p.grad.data_ptr() % 16 == 4 * offset for p in params)
            else:
                for p, g in zip(params, grads):
                    p.grad = g.clone()
            opt.step()
        runs.append([_bits(t) for p in params for t in (p, *(opt.state[p][k] for k in KEYS))])
        tab = chunk_table([(p.data_ptr(), p.grad.data_ptr(), 16, 32, 48, p.numel()) for p in params])
        assert set(tab["aligned"].tolist()) == ({1} if offset == 0 or not flat_views else {0})
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------ 4. special values
@pytest.mark.parametrize("weight_decay", [0.0, 1e-5])
def test_all_zero_gradients_from_a_zero_state(weight_decay):
    dev = _gpu()
    params, gen = _params(dev, [5, 4100], 31)
    pair = Pair("zero gradients wd%g" % weight_decay, params, dict(lr=1e-3, weight_decay=weight_decay, amsgrad=True))
    before = [_bits(p) for p in params]
    for _ in range(2):
        pair.step([torch.zeros_like(p) for p in params])
        pair.check()
    same = [torch.equal(a, _bits(p)) for a, p in zip(before, params)]
    assert all(same) if weight_decay == 0 else not any(same)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
def test_infinite_and_nan_gradients_poison_their_own_elements_only(aligned):
    dev = _gpu()
    n = 4100
    params, gen = _params(dev, [n], 37)
    pair = Pair("non-finite gradients", params, dict(lr=1e-3, weight_decay=1e-5, amsgrad=True))
    bad = {5: float("inf"), 6: float("-inf"), 2049: float("nan"), n - 1: float("inf")}
    flat = torch.zeros(n + 1, device=dev)
    for step in range(3):
        g = torch.randn(n, generator=gen)
        if step == 0:
            for i, v in bad.items():
                g[i] = v
        gv = flat[0 if aligned else 1:][:n]
        gv.copy_(g)
        pair.feed([g.to(dev)])
        params[0].grad = gv                                   # (the yardstick keeps its own aligned copy)
        pair.hip.step(); pair.torch.step()
        want = torch.zeros(n, dtype=torch.bool)
        want[list(bad)] = True
        sh, stt = pair.hip.state[params[0]], pair.torch.state[pair.tp[0]]
        for a, b in [(params[0], pair.tp[0])] + [(sh[k], stt[k]) for k in KEYS]:
            a, b = a.detach().cpu(), b.detach().cpu()
            assert torch.equal(~torch.isfinite(a), want) and torch.equal(torch.isnan(a), torch.isnan(b))
            assert torch.equal(a[torch.isinf(a)], b[torch.isinf(b)]) and torch.equal(torch.isinf(a), torch.isinf(b))
            ok = ~want
            assert float((a[ok] - b[ok]).abs().max()) <= 1e-6 * float(b[ok].abs().max())


def test_denormal_gradients_and_negative_zero():
    dev = _gpu()
    from bmc_hip.optim import Adam
    cfg = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=True)
    n = 4099
    gen = torch.Generator().manual_seed(41)
    p0 = torch.randn(n, generator=gen)
    p0[7] = -0.0
    g = (torch.randn(n, generator=gen) * 1e-40)
    assert float(g.abs().max()) < 1.2e-38 and float(g.abs().min()) > 0      # subnormal float32 values
    g[7] = -0.0
    g[8] = 0.0
    p = torch.nn.Parameter(p0.clone().to(dev))
    opt = Adam([p], **cfg)
    p.grad = g.to(dev)
    opt.step()
    st = opt.state[p]
    got = [t.detach().cpu().numpy() for t in (p, st["exp_avg"], st["exp_avg_sq"], st["max_exp_avg_sq"])]
    assert all(np.isfinite(a).all() for a in got)
    z = np.zeros(n, np.float32)
    want = _f32_step(p0.numpy(), g.numpy(), z, z, z, step=1.0, **cfg)
    for name, a, b in zip(("p",) + KEYS, got, want):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), name           # -0.0 / +0.0 and subnormals included
    assert np.signbit(got[0][7]) and got[0][7] == 0 and not np.signbit(got[1][7])   # p = -0.0 stays, m = 0 + 0.1 * (-0 - 0) = +0.0
    tp = torch.nn.Parameter(p0.clone().to(dev))
    ref = torch.optim.Adam([tp], foreach=False, **cfg)
    tp.grad = g.to(dev)
    ref.step()
    assert float((tp.detach().cpu() - p.detach().cpu()).abs().max()) <= 1e-7 * cfg["lr"] + 2e-7 * float(p0.abs().max())


# ------------------------------------------------------------------ 5. parameters without a gradient
def test_parameters_without_a_gradient_are_skipped():
    """One of three parameters has grad None in steps 2 and 3: its state and `step` stay put, the others advance, and step 4
    leaves as two launches (two step counts)."""
    dev = _gpu()
    from bmc_hip import optim
    params, gen = _params(dev, [300, 4097, 9], 43)
    pair = Pair("grad is None", params, dict(lr=1e-3, weight_decay=1e-5, amsgrad=True))
    launches = []
    for step in range(4):
        grads = _grads(gen, params)
        if step in (1, 2):
            frozen = [_bits(params[1])] + [_bits(pair.hip.state[params[1]][k]) for k in KEYS]
            grads[1] = None
        n0 = optim.STEP_LAUNCHES
        pair.step(grads)
        launches.append(optim.STEP_LAUNCHES - n0)
        pair.check()
        if step in (1, 2):
            now = [_bits(params[1])] + [_bits(pair.hip.state[params[1]][k]) for k in KEYS]
            assert all(torch.equal(a, b) for a, b in zip(frozen, now)) and float(pair.hip.state[params[1]]["step"]) == 1.0
    assert launches == [1, 1, 1, 2]
    assert [float(pair.hip.state[p]["step"]) for p in params] == [4.0, 2.0, 4.0] == [float(pair.torch.state[p]["step"]) for p in pair.tp]


# ------------------------------------------------------------------ 6. state interchange
@pytest.mark.parametrize("first", ["torch", "hip"])
def test_state_dicts_load_into_each_other(first):
    """Three steps with one optimizer, state_dict() -> load_state_dict() of the other, three more: within the bar of six
    torch steps.  The loaded state has torch's keys, dtypes and devices."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    cfg = dict(lr=1e-3, weight_decay=1e-5, amsgrad=True)
    params, gen = _params(dev, [300, 4097, 9], 47)
    pair = Pair("interchange, %s first" % first, params, cfg)          # pair.torch: six torch steps, the yardstick
    mixed_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    a = torch.optim.Adam(mixed_params, foreach=False, **cfg) if first == "torch" else Adam(mixed_params, **cfg)
    b = Adam(mixed_params, **cfg) if first == "torch" else torch.optim.Adam(mixed_params, foreach=False, **cfg)
    pair.hp, pair.hip = mixed_params, None
    for step in range(6):
        grads = _grads(gen, params)
        for p, g in zip(mixed_params, grads):
            p.grad = g.clone()
        if step == 3:
            sd = a.state_dict()
            assert sorted(sd["state"][0]) == sorted(("step",) + KEYS) and sd["state"][0]["step"].dtype == torch.float32
            assert not sd["state"][0]["step"].is_cuda and sd["state"][0]["exp_avg"].is_cuda
            b.load_state_dict(sd)
        (a if step < 3 else b).step()
        for p, g in zip(pair.tp, grads):
            p.grad = g.clone()
        pair.torch.step()
        pair.ref.step([g.cpu().numpy() for g in grads])
    pair.hip = b
    pair.check()
    assert [float(b.state[p]["step"]) for p in mixed_params] == [6.0] * 3


def test_checkpoint_round_trip_continues_bit_identically(tmp_path):
    """checkpoint.save_checkpoint / resume with the HIP optimizer (the toy model of tests/test_checkpoint.py, on the GPU)."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    from checkpoint import resume, save_checkpoint

    def toy():
        torch.manual_seed(0)
        m = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3)).to(dev)
        opt = Adam(m.parameters(), lr=1e-2, weight_decay=1e-5, amsgrad=True)
        return m, opt, torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.95)

    def train(m, opt, sch, steps, seed):
        g = torch.Generator().manual_seed(seed)
        for i in range(steps):
            x = torch.randn(4, 6, generator=g).to(dev)
            opt.zero_grad()
            m(x).pow(2).mean().backward()
            opt.step()
            if i % 2 == 1:
                sch.step()

    m, opt, sch = toy()
    train(m, opt, sch, 4, seed=1)
    path = str(tmp_path / "checkpoint-iteration4.pth")
    save_checkpoint(path, m, opt, sch, iteration=4, monitor_best=0.5)
    train(m, opt, sch, 3, seed=2)
    m2, opt2, sch2 = toy()
    assert resume(path, m2, opt2, sch2)["iteration"] == 4
    assert opt2.param_groups[0]["lr"] == pytest.approx(1e-2 * 0.95 ** 2)
    train(m2, opt2, sch2, 3, seed=2)
    for a, b in zip(m.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    for a, b in zip(m.parameters(), m2.parameters()):
        assert all(torch.equal(opt.state[a][k], opt2.state[b][k]) for k in KEYS) and float(opt2.state[b]["step"]) == 7.0


# ------------------------------------------------------------------ 7. parameter versions and the caches keyed on them
def test_parameter_versions_advance_and_the_next_forward_sees_the_new_weights():
    """BMCNet(4, 32, 1) at 12x20, B = 1: a bptt_step with the HIP optimizer, then a second forward pass.  The kernel writes the
    parameters behind autograd's back; without the version bump the second forward would run on the packed weights of the first."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    from infer import StreamingSR
    from models.BMCNet import BMCNet
    from test_gpu_r2 import rel_l2
    from train_step import bptt_step
    scale, n_c, n_b, B, L, H, W = 4, 32, 1, 1, 3, 12, 20
    gen = torch.Generator().manual_seed(53)
    inp = torch.poisson(torch.full((B, L, 2, H, W), 0.4), generator=gen).to(dev)
    gt = torch.poisson(torch.full((B, L, 2, scale * H, scale * W), 0.4), generator=gen).to(dev)

    def forward(m):
        z = lambda c: torch.zeros(B, c, H, W, device=dev)
        with torch.no_grad():
            return m(inp[:, 0:2].transpose(1, 2), z(n_c), z(n_c), z(n_c), z(2 * scale * scale), True)[-1].clone()

    preds = {}
    for kind in ("hip", "torch"):
        torch.manual_seed(54)
        m = BMCNet(scale, n_c, n_b).to(dev)
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(3.0)
        cfg = dict(lr=1e-2, weight_decay=1e-5, amsgrad=True)
        opt = Adam(m.parameters(), **cfg) if kind == "hip" else torch.optim.Adam(m.parameters(), **cfg)
        before = forward(m)
        sr = StreamingSR(m, n_c=n_c, scale=scale, graph=True)
        stamp, versions = sr._weights_stamp(), [p._version for p in m.parameters()]
        m.train()
        bptt_step(m, opt, inp, gt, n_c, scale)
        stepped = [i for i, p in enumerate(m.parameters()) if p.grad is not None]
        assert len(stepped) >= len(versions) - 2
        assert all(p._version > versions[i] for i, p in enumerate(m.parameters()) if i in stepped)
        assert sr._weights_stamp() != stamp
        preds[kind] = (before, forward(m))
    assert torch.equal(preds["hip"][0], preds["torch"][0])
    assert rel_l2(preds["hip"][1], preds["hip"][0]) > 1e-3              # the step moved the prediction ...
    assert rel_l2(preds["hip"][1], preds["torch"][1]) < 1e-5            # ... to where torch's Adam moves it


# ------------------------------------------------------------------ 8. hooks and schedulers
def test_lr_scheduler_changes_the_next_launch():
    dev = _gpu()
    params, gen = _params(dev, [300, 4097], 59)
    pair = Pair("StepLR", params, dict(lr=1e-2, weight_decay=1e-5, amsgrad=True))
    schedulers = [torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5) for o in (pair.hip, pair.torch)]
    for step in range(3):
        lr = 1e-2 * 0.5 ** step
        assert pair.hip.param_groups[0]["lr"] == pytest.approx(lr)
        pair.step(_grads(gen, params), lr=lr)
        pair.check(lr=lr)
        for s in schedulers:
            s.step()


def test_pre_step_hooks_of_the_reducer_and_of_ops_run():
    """GradAllReducer(model, opt) without a process group: its pre-step hook ran (the gradients are views of its flat buckets when
    the kernel reads them); the global pre-step hook bmc_hip.ops registers (weight gradients on the side stream) ran too."""
    dev = _gpu()
    from torch.optim.optimizer import _global_optimizer_pre_hooks
    from bmc_hip import ops
    from bmc_hip.optim import Adam
    from bmc_hip.parallel import GradAllReducer
    cfg = dict(lr=1e-3, weight_decay=1e-5, amsgrad=True)
    torch.manual_seed(61)
    m = torch.nn.Sequential(torch.nn.Linear(7, 33), torch.nn.Tanh(), torch.nn.Linear(33, 5)).to(dev)      # 7*33 = 231: odd offsets
    params = list(m.parameters())
    pair = Pair("GradAllReducer", params, cfg)
    red = GradAllReducer(m, pair.hip, bucket_mb=1.0)          # one bucket: offsets 0, 5, 170, 203
    assert len(pair.hip._optimizer_step_pre_hooks) == 1
    keys = [k for k, v in _global_optimizer_pre_hooks.items() if v is ops._join_before_step]
    assert len(keys) == 1
    calls = []
    _global_optimizer_pre_hooks[keys[0]] = lambda *a: (calls.append(a[0]), ops._join_before_step(*a))[1]
    try:
        x = torch.randn(4, 7, device=dev)
        for step in range(2):
            pair.hip.zero_grad()
            m(x).pow(2).mean().backward()
            grads = [p.grad.detach().clone() for p in params]
            pair.hip.step()
            for p in params:
                bi, off = red.slot[p]
                assert p.grad.data_ptr() == red.flat[bi].data_ptr() + 4 * off          # a bucket view: the reducer's hook ran
            assert any(p.grad.data_ptr() % 16 for p in params)
            for p, g in zip(pair.tp, grads):
                p.grad = g
            pair.torch.step()
            pair.ref.step([g.cpu().numpy() for g in grads])
            pair.check()
    finally:
        _global_optimizer_pre_hooks[keys[0]] = ops._join_before_step
        red.detach()
    assert [c for c in calls if c is pair.hip] == [pair.hip, pair.hip]


# ------------------------------------------------------------------ 9. inside a captured graph
def test_capturable_step_in_a_graph():
    """One eager step, one captured step replayed four times with the gradient buffers refilled in place: the device counter
    reads 5 and parameters and state are within the bar of five eager torch steps; a second identical run is bit-identical."""
    dev = _gpu()
    cfg = dict(lr=1e-3, weight_decay=1e-5, amsgrad=True)
    sizes = [5, 4097, 300]
    runs = []
    for run in range(2):
        params, gen = _params(dev, sizes, 67)
        pair = Pair("capturable", params, cfg, hip_kwargs=dict(capturable=True))
        all_grads = [_grads(gen, params) for _ in range(5)]
        static = [g.clone() for g in all_grads[0]]
        for p, g in zip(params, static):
            p.grad = g
        pair.hip.step()                                       # eager: tables and counters are made outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            pair.hip.step()
        for grads in all_grads[1:]:
            for s, g in zip(static, grads):
                s.copy_(g)
            graph.replay()
        torch.cuda.synchronize()
        counters = pair.hip.step_counter()
        assert len(counters) == 1 and counters[0].dtype == torch.int32 and int(counters[0].item()) == 5
        for p in params:
            st = pair.hip.state[p]["step"]
            assert st.is_cuda and st.dtype == torch.float32 and float(st) == 5.0
        for grads in all_grads:
            for p, g in zip(pair.tp, grads):
                p.grad = g.clone()
            pair.torch.step()
            pair.ref.step([g.cpu().numpy() for g in grads])
        pair.check()
        runs.append([_bits(t) for p in params for t in (p, *(pair.hip.state[p][k] for k in KEYS))])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------ 10. the gradient norm
def _norm_check(dev, params, grads):
    from bmc_hip.optim import Adam
    want = float(np.sqrt(sum(float((g.double().cpu() ** 2).sum()) for g in grads)))
    got = []
    for _ in range(2):
        ps = [torch.nn.Parameter(p.detach().clone()) for p in params]
        opt = Adam(ps, lr=1e-4, weight_decay=1e-5, amsgrad=True, track_grad_norm=True)
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        n = opt.grad_norm()
        assert n.dtype == torch.float64 and n.is_cuda and n.dim() == 0
        got.append(n.cpu())
    assert abs(float(got[0]) - want) <= 1e-9 * want, (float(got[0]), want)
    assert torch.equal(got[0].view(torch.int64), got[1].view(torch.int64))


def test_grad_norm_of_the_size_cases():
    dev = _gpu()
    from bmc_hip.optim import Adam
    params, gen = _params(dev, SIZES, 71)
    grads = _grads(gen, params)
    _norm_check(dev, params, grads)
    flat = torch.zeros(sum(SIZES) + 1, device=dev)            # ... and through the one-by-one path: the same norm to 1e-9
    ps = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt = Adam(ps, lr=1e-4, track_grad_norm=True)
    at = 1
    for p, g in zip(ps, grads):
        flat[at:at + p.numel()].copy_(g)
        p.grad = flat[at:at + p.numel()]
        at += p.numel()
    opt.step()
    want = float(np.sqrt(sum(float((g.double().cpu() ** 2).sum()) for g in grads)))
    assert abs(float(opt.grad_norm()) - want) <= 1e-9 * want
    off = Adam([torch.nn.Parameter(p.detach().clone()) for p in params], lr=1e-4)
    for p, g in zip(off.param_groups[0]["params"], grads):
        p.grad = g.clone()
    off.step()
    assert all(entry[2] is None for entry in off._memo.values()) and off._norm_parts is None       # no partials are allocated
    with pytest.raises(RuntimeError, match="track_grad_norm"):
        off.grad_norm()


def test_grad_norm_of_the_bmcnet_parameter_set():
    dev = _gpu()
    from models.BMCNet import BMCNet
    torch.manual_seed(73)
    params = [p.detach().to(dev) for p in BMCNet(4, 128, 5).parameters()]
    assert len(params) == 54 and sum(p.numel() for p in params) == 2731680
    gen = torch.Generator().manual_seed(74)
    _norm_check(dev, params, _grads(gen, params))


# ------------------------------------------------------------------ 11. refusals
def test_refusals_on_the_device():
    dev = _gpu()
    from bmc_hip import lib, optim
    from bmc_hip.optim import Adam
    w = lambda *shape, **kw: torch.nn.Parameter(torch.zeros(*(shape or (3, 2)), device=dev, **kw))
    with pytest.raises(ValueError, match="float32"):
        Adam([w(dtype=torch.bfloat16)])
    with pytest.raises(ValueError, match="float32"):
        Adam([w(dtype=torch.float64)])
    with pytest.raises(ValueError, match="contiguous"):
        Adam([torch.nn.Parameter(torch.zeros(3, 2, device=dev).t())])
    for flag in ("maximize", "foreach", "fused", "differentiable", "decoupled_weight_decay"):
        with pytest.raises(ValueError, match=flag):
            Adam([w()], **{flag: True})
        opt = Adam([w()])
        opt.param_groups[0][flag] = True                     # ... or arriving later, e.g. through load_state_dict
        opt.param_groups[0]["params"][0].grad = torch.zeros(3, 2, device=dev)
        with pytest.raises(ValueError, match=flag):
            opt.step()
    with pytest.raises(ValueError, match="tensor lr"):
        Adam([w()], lr=torch.tensor(1e-3, device=dev))
    opt = Adam([w()])
    opt.param_groups[0]["lr"] = torch.tensor(1e-3)
    opt.param_groups[0]["params"][0].grad = torch.zeros(3, 2, device=dev)
    with pytest.raises(ValueError, match="tensor lr"):
        opt.step()
    # gradients: sparse; another shape, dtype or device than the parameter's (torch refuses most of these at `p.grad = ...`
    # already; `.grad.data = ...` is the way around it that a careless caller has)
    p = w(4, 3)
    opt = Adam([("head.weight", p)])
    p.grad = torch.zeros(4, 3, device=dev).to_sparse()
    n0 = optim.STEP_LAUNCHES
    with pytest.raises(ValueError, match="'head.weight'.*sparse"):
        opt.step()
    for bad in (torch.zeros(3, 4, device=dev), torch.zeros(4, 3, device=dev, dtype=torch.float64), torch.zeros(4, 3),
                torch.zeros(3, 4, device=dev).t()):
        p.grad = torch.zeros(4, 3, device=dev)
        try:
            p.grad.data = bad
        except (RuntimeError, TypeError):
            continue                                          # this torch closes the route itself
        with pytest.raises(ValueError, match="'head.weight'"):
            opt.step()
    assert optim.STEP_LAUNCHES == n0 and len(opt.state[p]) == 0
    # the C ABI: a NULL table with two chunks, a NaN eps, a negative count -- the error code and a message, nothing is launched
    h = optim.step_hyper(1e-3, 0.9, 0.999, 1e-8, 0.0, True, 1.0)
    assert lib._adam_step(None, 2, h, None, None) < 0 and b"no chunk table" in lib.bmc_last_error()
    assert lib._adam_step(None, -1, h, None, None) < 0 and b"negative" in lib.bmc_last_error()
    assert lib._adam_step(None, 0, h, None, None) == 0
    table = torch.zeros(48, dtype=torch.uint8, device=dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    h = optim.step_hyper(1e-3, 0.9, 0.999, float("nan"), 0.0, True, 1.0)
    assert lib._adam_step(table.data_ptr(), 1, h, None, None) < 0 and b"not finite" in lib.bmc_last_error()
    assert lib._adam_step_cap(table.data_ptr(), 1, h, step_dev.data_ptr(), None, None) < 0 and b"not finite" in lib.bmc_last_error()
    h = optim.step_hyper(float("inf"), 0.9, 0.999, 1e-8, 0.0, True, None)
    assert lib._adam_step_cap(table.data_ptr(), 1, h, step_dev.data_ptr(), None, None) < 0 and b"not finite" in lib.bmc_last_error()
    assert lib._adam_step_cap(None, 2, optim.step_hyper(1e-3, 0.9, 0.999, 1e-8, 0.0, True, None), step_dev.data_ptr(), None, None) < 0
    torch.cuda.synchronize()
    assert int(step_dev.item()) == 0


def test_step_returns_the_closure_loss_and_copies_the_table_once():
    dev = _gpu()
    from bmc_hip import optim
    from bmc_hip.optim import Adam
    p = torch.nn.Parameter(torch.ones(5000, device=dev))
    opt = Adam([p], lr=1e-2)

    def closure():
        opt.zero_grad(set_to_none=False)
        loss = (p * p).sum()
        loss.backward()
        return loss

    p.grad = torch.zeros_like(p)
    n0 = optim.TABLE_COPIES
    losses = [float(opt.step(closure).detach()) for _ in range(4)]
    assert losses == sorted(losses, reverse=True) and losses[0] == 5000.0 and losses[-1] < losses[0]
    assert optim.TABLE_COPIES == n0 + 1                        # the same buffers: the memoised table
