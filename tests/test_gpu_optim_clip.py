"""bmc_hip.optim.Adam(max_grad_norm=, nonfinite=) on the MI355X (csrc/optim_clip.hip, include/bmc_hip.h "optimizer step: clipping").

The yardstick is torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False) followed by torch.optim.Adam(foreach=False) in fp32
on the same GPU; both sides are measured against the float64 restatement of tests/optim_clip_ref.py with e(x) of
tests/test_gpu_optim.py, and the bar is that file's with one term for the coefficient's three float32 roundings:
    e_hip <= 2 * e_torch + 1e-7 + E_c      E_c = 2^-22 for p and exp_avg (linear in c), 2^-21 for exp_avg_sq and max_exp_avg_sq
(3 * 2^-24 rounded up to a power of two; twice that where c enters squared).  On top of that every clipped step is compared BIT FOR
BIT with the numpy float32 evaluation g * c followed by the six lines (_f32_step of tests/test_gpu_optim.py), c read back from the
device, and c itself with the numpy float32 coefficient function applied to the device's float64 norm.

Tensors are views of NaN-guarded buffers (aligned and packed), sizes 1 .. 12293, gradient scales 1e-8, 1e-4, 1, 1e3 across tensors;
the guards are checked after every test that uses them.

Measured (MI355X, this file, test_against_the_yardstick; the largest value over tensors and the five steps, printed with -s):
  (e_hip / e_torch; aligned = packed)  p                    exp_avg              exp_avg_sq           max_exp_avg_sq
  amsgrad on,  wd 0                    5.01e-03 / 5.01e-03  2.86e-07 / 1.19e-08  2.26e-07 / 2.26e-07  2.26e-07 / 2.26e-07
  amsgrad on,  wd 1e-5                 5.01e-03 / 5.01e-03  1.68e-07 / 1.32e-07  2.06e-07 / 2.10e-07  2.06e-07 / 2.10e-07
  amsgrad off, wd 0                    5.01e-03 / 5.01e-03  2.86e-07 / 1.19e-08  2.26e-07 / 2.26e-07  -
  amsgrad off, wd 1e-5                 5.01e-03 / 5.01e-03  1.68e-07 / 1.32e-07  2.06e-07 / 2.10e-07  -
exp_avg without weight decay is where the E_c term is needed: torch's coefficient happens to round well on these gradients
(e_torch 1.2e-8), ours carries the three roundings (2.9e-7 against a bar of 2 * 1.2e-8 + 1e-7 + 2.4e-7 = 3.6e-7).  e(p) is the
rounding of p itself, the same for both.  torch.cuda.set_sync_debug_mode("error") works in this ROCm build (the probe raises).
"""

import numpy as np
import pytest
import torch

import optim_clip_ref as CR
import optim_ref as R
from test_gpu_optim import GUARD, KEYS, SCALES, SIZES, _bits, _f32_step, _grads, _guarded, _params, _setting_id  # noqa: F401
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401

pytestmark = pytest.mark.gpu

E_C = {"p": 2.0 ** -22, "exp_avg": 2.0 ** -22, "exp_avg_sq": 2.0 ** -21, "max_exp_avg_sq": 2.0 ** -21}
WORST = {}
LAYOUTS = pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "packed"])


@pytest.fixture(scope="module", autouse=True)
def _print_measured():
    yield
    for name, row in WORST.items():
        print("\n%-34s " % name + "  ".join("%s %.2e / %.2e" % (k, a, b) for k, (a, b) in sorted(row.items())), end="")
    print()


class Rig:
    """p, exp_avg, exp_avg_sq, max_exp_avg_sq and the gradients as views of five NaN-guarded buffers."""

    def __init__(self, dev, aligned, seed, sizes=SIZES):
        self.gen = torch.Generator().manual_seed(seed)
        self.bufs = [_guarded(dev, sizes, aligned) for _ in range(5)]        # p, m, v, vmax, g
        for t in self.bufs[0][2]:
            t.copy_(torch.randn(t.shape, generator=self.gen))
        for _, _, views in self.bufs[1:]:
            for t in views:
                t.zero_()
        self.params = [torch.nn.Parameter(t) for t in self.bufs[0][2]]
        assert all(p.data_ptr() == t.data_ptr() for p, t in zip(self.params, self.bufs[0][2]))
        assert aligned == all(t.data_ptr() % 16 == 0 for b in self.bufs for t in b[2])
        for p, g in zip(self.params, self.bufs[4][2]):
            p.grad = g

    def install_state(self, opt, amsgrad):
        for i, p in enumerate(self.params):
            st = dict(step=torch.tensor(0.0), exp_avg=self.bufs[1][2][i], exp_avg_sq=self.bufs[2][2][i])
            if amsgrad:
                st["max_exp_avg_sq"] = self.bufs[3][2][i]
            opt.state[p] = st

    def feed(self, grads):
        for view, g in zip(self.bufs[4][2], grads):
            view.copy_(g)

    def snapshot(self, which=range(5)):
        torch.cuda.synchronize()
        return [self.bufs[k][0].view(torch.int32).clone() for k in which]

    def guards_untouched(self):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(buf[mask]).all()) for buf, mask, _ in self.bufs)


class F32:
    """The numpy float32 evaluation: g * c (one rounding), then the six lines; one step count and one configuration per tensor."""

    def __init__(self, params, cfgs):
        self.cfgs = cfgs
        self.t = [[p.detach().cpu().numpy().reshape(-1).copy()] + [np.zeros(p.numel(), np.float32) for _ in range(3)] for p in params]
        self.steps = [0] * len(params)

    def step(self, grads, c):
        c = np.float32(c)
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.steps[i] += 1
            with np.errstate(all="ignore"):
                gc = g.detach().cpu().numpy().reshape(-1) * c
            self.t[i] = list(_f32_step(self.t[i][0], gc, *self.t[i][1:], step=float(self.steps[i]), **self.cfgs[i]))

    def check(self, params, opt, where=""):
        """bit for bit; where the evaluation is NaN the device must be NaN (sign and payload of a NaN are not compared)"""
        for i, p in enumerate(params):
            if self.steps[i] == 0:
                continue
            st = opt.state[p]
            got = [p, st["exp_avg"], st["exp_avg_sq"]] + ([st["max_exp_avg_sq"]] if self.cfgs[i]["amsgrad"] else [])
            for name, a, b in zip(("p",) + KEYS, got, self.t[i]):
                a = a.detach().cpu().numpy().reshape(-1)
                nan = np.isnan(b)
                assert np.array_equal(np.isnan(a), nan), (where, i, name)
                assert np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan]), (where, i, name)


def _cfg(setting, lr=1e-4):
    return dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, **setting)


def _clip_of(opt):
    torch.cuda.synchronize()
    norm, c = opt.last_clip().cpu().tolist()
    return norm, c


def _rel(a, b):
    return abs(a - b) / abs(b)


# ------------------------------------------------------------------ 1. the norm launch through the C ABI
@LAYOUTS
def test_norm_launch_equals_the_step_launch_partials(aligned):
    """bmc_adam_grad_sq and bmc_adam_step(..., partial_sq, ...) over ONE chunk table (bmc_hip.optim.chunk_table over the guarded
    views): the same float64 bits per chunk; the norm launch leaves p, m, v, vmax and g byte-identical."""
    dev = _gpu()
    from bmc_hip import lib, optim
    rig = Rig(dev, aligned, 101)
    rig.feed(_grads(rig.gen, rig.params))
    for t in rig.bufs[2][2] + rig.bufs[3][2]:
        t.copy_(torch.rand(t.shape, generator=rig.gen))
    tab = optim.chunk_table([tuple(rig.bufs[k][2][i].data_ptr() for k in (0, 4, 1, 2, 3)) + (n,) for i, n in enumerate(SIZES)])
    assert len(tab) == sum((n + 4095) // 4096 for n in SIZES)
    assert set(tab["aligned"].tolist()) == {1} if aligned else 0 in tab["aligned"][1:].tolist()
    table = torch.from_numpy(tab.view(np.uint8).reshape(-1).copy()).to(dev)
    a = torch.full((len(tab) + 2,), -1.0, dtype=torch.float64, device=dev)       # one sentinel before and after
    b = torch.full((len(tab),), -2.0, dtype=torch.float64, device=dev)
    before = rig.snapshot()
    assert lib._adam_grad_sq(table.data_ptr(), len(tab), a.data_ptr() + 8, None) == 0
    after = rig.snapshot()
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    h = optim.step_hyper(1e-4, 0.9, 0.999, 1e-8, 1e-5, True, 1.0)
    assert lib._adam_step(table.data_ptr(), len(tab), h, b.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(a[1:-1].view(torch.int64), b.view(torch.int64)) and float(a[0]) == -1.0 and float(a[-1]) == -1.0
    assert float(b.sum().sqrt()) == pytest.approx(CR.global_norm64([g.cpu().numpy() for g in rig.bufs[4][2]]), rel=1e-12)
    assert not torch.equal(rig.snapshot([0])[0], before[0])                      # (the step launch did move p)
    assert rig.guards_untouched()


# ------------------------------------------------------------------ 2. coefficient and norm
@LAYOUTS
@pytest.mark.parametrize("max_norm", [1e3, 1e7], ids=["clipping", "not_clipping"])
def test_norm_and_coefficient(max_norm, aligned):
    """last_clip()[0] against math.fsum over the exact squares (1e-12 relative); float32(last_clip()[1]) is the numpy float32
    coefficient function of last_clip()[0], bit for bit.  grad_norm() reads the same partials."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    rig = Rig(dev, aligned, 103)
    opt = Adam(rig.params, max_grad_norm=max_norm, **_cfg(dict(amsgrad=True, weight_decay=1e-5)))
    rig.install_state(opt, True)
    for _ in range(2):
        grads = _grads(rig.gen, rig.params)
        rig.feed(grads)
        opt.step()
        norm, c = _clip_of(opt)
        info = opt.last_clip()
        assert info.dtype == torch.float64 and info.is_cuda and tuple(info.shape) == (2,)
        want = CR.global_norm64([g.cpu().numpy() for g in grads])
        assert _rel(norm, want) <= 1e-12, (norm, want)
        assert np.float32(c).view(np.int32) == CR.coeff32(norm, max_norm).view(np.int32) and float(np.float32(c)) == c
        assert (c < 1.0) == (max_norm < want) and _rel(float(opt.grad_norm()), want) <= 1e-12
    assert int(opt.skipped_steps()) == 0 and opt.skipped_steps().dtype == torch.int32 and opt.skipped_steps().dim() == 0
    assert rig.guards_untouched()


# ------------------------------------------------------------------ 3. an inactive clip is invisible
@LAYOUTS
@pytest.mark.parametrize("kwargs", [dict(max_grad_norm=1e30), dict(max_grad_norm=None, nonfinite="skip")], ids=["1e30", "guard_only"])
def test_inactive_clip_is_invisible(kwargs, aligned):
    """c == 1.0 exactly, and over three steps p and the three state tensors equal an unclipped bmc_hip.optim.Adam on copies."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    cfg = _cfg(dict(amsgrad=True, weight_decay=1e-5))
    rig = Rig(dev, aligned, 107)
    plain_params = [torch.nn.Parameter(p.detach().clone()) for p in rig.params]
    opt, plain = Adam(rig.params, **cfg, **kwargs), Adam(plain_params, **cfg)
    rig.install_state(opt, True)
    for step in range(3):
        grads = _grads(rig.gen, rig.params)
        rig.feed(grads)
        for p, g in zip(plain_params, grads):
            p.grad = g.clone()
        opt.step(); plain.step()
        assert _clip_of(opt)[1] == 1.0
        for p, q in zip(rig.params, plain_params):
            assert torch.equal(_bits(p), _bits(q)), step
            assert all(torch.equal(_bits(opt.state[p][k]), _bits(plain.state[q][k])) for k in KEYS), step
    assert int(opt.skipped_steps()) == 0 and rig.guards_untouched()


# ------------------------------------------------------------------ 4. an active clip, bit for bit
@LAYOUTS
@pytest.mark.parametrize("setting", R.SETTINGS, ids=_setting_id)
def test_active_clip_bit_for_bit(setting, aligned):
    """max_grad_norm = 1e3 below a norm of about 1.1e5: every step equals g * c and the six lines in numpy float32, c read back
    from the device; .grad is byte-identical after step() (the kernel multiplies while it reads)."""
    dev = _gpu()
    from bmc_hip import optim
    cfg = _cfg(setting)
    rig = Rig(dev, aligned, 109)
    opt = optim.Adam(rig.params, max_grad_norm=1e3, **cfg)
    rig.install_state(opt, setting["amsgrad"])
    f32 = F32(rig.params, [cfg] * len(SIZES))
    for step in range(3):
        grads = _grads(rig.gen, rig.params)
        rig.feed(grads)
        g_before = rig.snapshot([4])[0]
        n0, s0 = optim.NORM_LAUNCHES, optim.STEP_LAUNCHES
        opt.step()
        assert (optim.NORM_LAUNCHES, optim.STEP_LAUNCHES) == (n0 + 1, s0 + 1)
        norm, c = _clip_of(opt)
        assert 0.0 < c < 0.05 and np.float32(c) == CR.coeff32(norm, 1e3)
        assert torch.equal(rig.snapshot([4])[0], g_before)
        f32.step(grads, c)
        f32.check(rig.params, opt, "step %d" % step)
    assert rig.guards_untouched()
    if not setting["amsgrad"]:
        assert all(bool((t == 0).all()) for t in rig.bufs[3][2])


# ------------------------------------------------------------------ 5. against the yardstick
@LAYOUTS
@pytest.mark.parametrize("setting", R.SETTINGS, ids=_setting_id)
def test_against_the_yardstick(setting, aligned):
    """Five steps, max_norm = 1e4: the gradients of steps 1 and 2 are a hundred times smaller than those of steps 3 to 5, so the
    first two are not clipped (norm about 1.1e3) and the last three are (norm about 1.1e5, c about 0.09)."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    cfg, max_norm = _cfg(setting), 1e4
    rig = Rig(dev, aligned, 113)
    tp = [torch.nn.Parameter(p.detach().clone()) for p in rig.params]
    hip = Adam(rig.params, max_grad_norm=max_norm, **cfg)
    rig.install_state(hip, setting["amsgrad"])
    yard = torch.optim.Adam(tp, foreach=False, **cfg)
    ref = CR.ClippedAdam64([p.detach().cpu().numpy() for p in rig.params], max_norm, **cfg)
    row = WORST.setdefault("%s %s" % (_setting_id(setting), "aligned" if aligned else "packed"), {})
    clipped = []
    for step in range(5):
        grads = [g * (0.01 if step < 2 else 1.0) for g in _grads(rig.gen, rig.params)]
        rig.feed(grads)
        for p, g in zip(tp, grads):
            p.grad = g.clone()
        hip.step()
        torch.nn.utils.clip_grad_norm_(tp, max_norm, foreach=False)
        yard.step()
        ref.step([g.cpu().numpy() for g in grads])
        clipped.append(_clip_of(hip)[1] < 1.0)
        assert _rel(_clip_of(hip)[1], ref.last[1]) <= 3 * 2.0 ** -24
        for i, (ph, pt) in enumerate(zip(rig.params, tp)):
            pairs = [("p", R.e_param(ph, ref.p[i], cfg["lr"]), R.e_param(pt, ref.p[i], cfg["lr"]))]
            sh, stt = hip.state[ph], yard.state[pt]
            for key, x64 in zip(KEYS, (ref.m[i], ref.v[i], ref.vmax[i])):
                if key in stt:
                    pairs.append((key, R.e_state(sh[key], x64), R.e_state(stt[key], x64)))
            for key, eh, et in pairs:
                if eh >= row.get(key, (-1.0, 0.0))[0]:
                    row[key] = (eh, et)
                assert eh <= 2 * et + 1e-7 + E_C[key], (step, "tensor %d" % i, key, "e_hip %.3e" % eh, "e_torch %.3e" % et)
    assert clipped == [False, False, True, True, True] and rig.guards_untouched()


# ------------------------------------------------------------------ 6. several launches, one norm
def test_several_launches_share_one_global_norm():
    """Two groups (lr 1e-3 and 1e-2) and one parameter of the first group that has no gradient in step 1: two step launches in
    step 1, three in steps 2 and 3 (two step-count cohorts in the first group), as many norm launches, ONE coefficient."""
    dev = _gpu()
    from bmc_hip import optim
    sizes = [300, 4097, 9, 5000, 7]
    params, gen = _params(dev, sizes, 127)
    base = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, amsgrad=True)
    opt = optim.Adam([dict(params=params[:3], lr=1e-3), dict(params=params[3:], lr=1e-2)], max_grad_norm=1.0, **base)
    f32 = F32(params, [dict(base, lr=1e-3)] * 3 + [dict(base, lr=1e-2)] * 2)
    grew = []
    for step in range(3):
        grads = _grads(gen, params, scales=[1e-2, 1.0, 1e-1])
        if step == 0:
            grads[1] = None
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.clone()
        n0, s0 = optim.NORM_LAUNCHES, optim.STEP_LAUNCHES
        opt.step()
        grew.append((optim.NORM_LAUNCHES - n0, optim.STEP_LAUNCHES - s0))
        norm, c = _clip_of(opt)
        assert _rel(norm, CR.global_norm64([None if g is None else g.cpu().numpy() for g in grads])) <= 1e-12       # ALL gradients
        assert np.float32(c) == CR.coeff32(norm, 1.0) and c < 1.0
        f32.step(grads, c)
        f32.check(params, opt, "step %d" % step)
    assert grew == [(2, 2), (3, 3), (3, 3)]
    assert [float(opt.state[p]["step"]) for p in params] == [3.0, 2.0, 3.0, 3.0, 3.0]


# ------------------------------------------------------------------ 7. nonfinite="propagate"
@LAYOUTS
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")], ids=["inf", "neg_inf", "nan"])
def test_nonfinite_propagate(bad, aligned):
    """One Inf element: c == 0, that element's parameter becomes NaN (Inf * 0), every other follows the evaluation with g_c = 0.
    One NaN element: c is NaN and everything becomes NaN.  This is clip_grad_norm_(error_if_nonfinite=False) before step()."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    cfg = _cfg(dict(amsgrad=True, weight_decay=1e-5))
    rig = Rig(dev, aligned, 131)
    opt = Adam(rig.params, max_grad_norm=1e3, **cfg)
    rig.install_state(opt, True)
    f32 = F32(rig.params, [cfg] * len(SIZES))
    grads = _grads(rig.gen, rig.params)
    grads[6][4096] = bad                                      # the one-by-one tail of the aligned path, the second chunk
    rig.feed(grads)
    opt.step()
    norm, c = _clip_of(opt)
    if np.isnan(bad):
        assert np.isnan(norm) and np.isnan(c)
        assert all(bool(torch.isnan(t).all()) for p in rig.params for t in (p, *(opt.state[p][k] for k in KEYS)))
    else:
        assert norm == float("inf") and c == 0.0
        nan = [torch.isnan(p.detach()).nonzero().flatten().tolist() for p in rig.params]
        assert nan == [[]] * 6 + [[4096]] + [[]]
    f32.step(grads, c)
    f32.check(rig.params, opt)
    assert int(opt.skipped_steps()) == 0 and rig.guards_untouched()


# ------------------------------------------------------------------ 8. nonfinite="skip"
@LAYOUTS
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_skip(bad, aligned):
    """The step with one bad element stores nothing to p, m, v, vmax; skipped_steps() reads 1; the next step, with finite
    gradients, is the evaluation at step count 2 from the untouched state (a skipped step counts as a step)."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    cfg = _cfg(dict(amsgrad=True, weight_decay=1e-5))
    rig = Rig(dev, aligned, 137)
    opt = Adam(rig.params, max_grad_norm=1e3, nonfinite="skip", **cfg)
    rig.install_state(opt, True)
    for k in (1, 2, 3):                                       # a state that is not all zero, between the same guards
        for t in rig.bufs[k][2]:
            t.copy_(torch.rand(t.shape, generator=rig.gen) * 1e-3)
    f32 = F32(rig.params, [cfg] * len(SIZES))
    for i in range(len(SIZES)):
        f32.t[i][1:] = [rig.bufs[k][2][i].cpu().numpy().copy() for k in (1, 2, 3)]
    versions = [p._version for p in rig.params]
    grads = _grads(rig.gen, rig.params)
    grads[7][12292] = bad                                     # the very last element of the last chunk
    rig.feed(grads)
    before = rig.snapshot()
    opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, rig.snapshot()))
    assert int(opt.skipped_steps()) == 1 and not np.isfinite(_clip_of(opt)[0])
    assert all(p._version > v for p, v in zip(rig.params, versions))             # versions advance after a skipped step too
    assert [float(opt.state[p]["step"]) for p in rig.params] == [1.0] * len(SIZES)
    grads = _grads(rig.gen, rig.params)
    rig.feed(grads)
    opt.step()
    norm, c = _clip_of(opt)
    assert np.isfinite(norm) and 0.0 < c < 1.0 and int(opt.skipped_steps()) == 1
    f32.steps = [1] * len(SIZES)                              # the skipped step counted
    f32.step(grads, c)
    f32.check(rig.params, opt)
    assert [float(opt.state[p]["step"]) for p in rig.params] == [2.0] * len(SIZES) == [float(s) for s in f32.steps]
    assert rig.guards_untouched()


# ------------------------------------------------------------------ 9. inside a captured graph
def test_clipped_capturable_step_in_a_graph():
    """capturable=True, nonfinite="skip": one eager step, then [norm, step, advance] captured once and replayed three times with new
    gradients copied into the static .grad buffers, the second replay carrying an Inf -- bit-identical to the same four steps taken
    eagerly.  Every launch of step() goes to the current stream, one after the other: the capture is a single chain (one norm
    launch, one step launch counted while capturing)."""
    dev = _gpu()
    from bmc_hip import optim
    cfg = dict(lr=1e-3, weight_decay=1e-5, amsgrad=True)
    sizes = [5, 4097, 300]

    def run(graphed):
        params, gen = _params(dev, sizes, 139)
        opt = optim.Adam(params, capturable=True, max_grad_norm=20.0, nonfinite="skip", **cfg)
        all_grads = [_grads(gen, params, scales=[1e-2, 1.0, 1e-1]) for _ in range(4)]
        all_grads[2][1][4096] = float("inf")
        static = [g.clone() for g in all_grads[0]]
        for p, g in zip(params, static):
            p.grad = g
        opt.step()
        torch.cuda.synchronize()
        if graphed:
            graph = torch.cuda.CUDAGraph()
            n0, s0, t0 = optim.NORM_LAUNCHES, optim.STEP_LAUNCHES, optim.TABLE_COPIES
            with torch.cuda.graph(graph):
                opt.step()
            assert (optim.NORM_LAUNCHES, optim.STEP_LAUNCHES, optim.TABLE_COPIES) == (n0 + 1, s0 + 1, t0)
        clips = []
        for grads in all_grads[1:]:
            for s, g in zip(static, grads):
                s.copy_(g)
            graph.replay() if graphed else opt.step()
            clips.append(_clip_of(opt))
        counters = opt.step_counter()
        assert len(counters) == 1 and int(counters[0].item()) == 4 and int(opt.skipped_steps()) == 1
        assert all(float(opt.state[p]["step"]) == 4.0 for p in params)
        assert [np.isfinite(n) for n, _ in clips] == [True, False, True] and all(c < 1.0 for _, c in (clips[0], clips[2]))
        return [_bits(t) for p in params for t in (p, *(opt.state[p][k] for k in KEYS))], clips

    (a, ca), (b, cb) = run(True), run(False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert [c for _, c in ca] == [c for _, c in cb] and ca[0] == cb[0] and ca[2] == cb[2]


# ------------------------------------------------------------------ 10. GradAllReducer on one rank
def test_clipping_reads_the_reducers_buckets_and_leaves_them():
    """GradAllReducer(model, opt) without a process group, as test_pre_step_hooks_of_the_reducer_and_of_ops_run uses it: when the
    norm launch runs the gradients are (unaligned) views of the flat bucket; the norm is theirs; the bucket holds the reduced
    gradients, byte for byte, after the step (torch's clip_grad_norm_ would have scaled them in place)."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    from bmc_hip.parallel import GradAllReducer
    cfg = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, amsgrad=True)
    torch.manual_seed(61)
    m = torch.nn.Sequential(torch.nn.Linear(7, 33), torch.nn.Tanh(), torch.nn.Linear(33, 5)).to(dev)      # 7*33 = 231: odd offsets
    params = list(m.parameters())
    max_norm = 1e-3
    opt = Adam(params, max_grad_norm=max_norm, **cfg)
    red = GradAllReducer(m, opt, bucket_mb=1.0)
    f32 = F32(params, [cfg] * len(params))
    try:
        x = torch.randn(4, 7, device=dev)
        for step in range(2):
            opt.zero_grad()
            m(x).pow(2).mean().backward()
            grads = [p.grad.detach().clone() for p in params]
            opt.step()
            for p, g in zip(params, grads):
                bi, off = red.slot[p]
                assert p.grad.data_ptr() == red.flat[bi].data_ptr() + 4 * off
                assert torch.equal(_bits(red.flat[bi][off:off + p.numel()]), _bits(g.reshape(-1)))
            assert any(p.grad.data_ptr() % 16 for p in params)
            norm, c = _clip_of(opt)
            assert _rel(norm, CR.global_norm64([g.cpu().numpy() for g in grads])) <= 1e-12
            assert c < 1.0 and np.float32(c) == CR.coeff32(norm, max_norm)
            f32.step(grads, c)
            f32.check(params, opt, "step %d" % step)
    finally:
        red.detach()


# ------------------------------------------------------------------ 11. no host round trip
def test_clipped_step_makes_no_host_round_trip():
    """The second and third step() of a non-capturable clipped optimizer under torch.cuda.set_sync_debug_mode("error"); the mode is
    first shown to work in this build (an .item() on a device tensor raises).  Besides: no chunk table is copied again."""
    dev = _gpu()
    from bmc_hip import optim
    params, gen = _params(dev, [300, 4097, 9], 151)
    opt = optim.Adam(params, lr=1e-3, weight_decay=1e-5, amsgrad=True, max_grad_norm=1.0, nonfinite="skip", track_grad_norm=True)
    grads = _grads(gen, params)
    for p, g in zip(params, grads):
        p.grad = g
    opt.step()
    torch.cuda.synchronize()
    copies = optim.TABLE_COPIES
    probe = torch.ones(1, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        opt.step()
        opt.step()
        info, skipped, norm = opt.last_clip(), opt.skipped_steps(), opt.grad_norm()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert optim.TABLE_COPIES == copies
    assert float(info[1]) < 1.0 and int(skipped) == 0 and _rel(float(norm), float(info[0])) <= 1e-12


# ------------------------------------------------------------------ 12. state interchange
def test_state_dict_is_that_of_an_unclipped_optimizer():
    """(gradient scales 1e-8 and 1e-4: a norm of about 6e-3, clipped at 1e-3)"""
    dev = _gpu()
    from bmc_hip.optim import Adam
    cfg = dict(lr=1e-3, weight_decay=1e-5, amsgrad=True)
    params, gen = _params(dev, [300, 4097], 157)
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    clipped, plain = Adam(params, max_grad_norm=1e-3, nonfinite="skip", **cfg), Adam(twins, **cfg)
    grads = _grads(gen, params)
    for ps in (params, twins):
        for p, g in zip(ps, grads):
            p.grad = g.clone()
    clipped.step(); plain.step()
    a, b = clipped.state_dict(), plain.state_dict()
    assert [sorted(g) for g in a["param_groups"]] == [sorted(g) for g in b["param_groups"]]
    assert {k: sorted(v) for k, v in a["state"].items()} == {k: sorted(v) for k, v in b["state"].items()}
    assert not any("norm" in k or "nonfinite" in k for g in a["param_groups"] for k in g)
    yard = torch.optim.Adam(params, foreach=False, **cfg)
    yard.load_state_dict(a)
    yard.step()
    back = Adam(params, max_grad_norm=1e-3, nonfinite="skip", **cfg)
    back.load_state_dict(yard.state_dict())
    back.step()
    assert [float(back.state[p]["step"]) for p in params] == [3.0, 3.0] and back.max_grad_norm == 1e-3 and back.nonfinite == "skip"
    assert _clip_of(back)[1] < 1.0 and all(bool(torch.isfinite(p).all()) for p in params)


# ------------------------------------------------------------------ 13. refusals
def test_clip_refusals_on_the_device():
    dev = _gpu()
    from bmc_hip import lib, optim
    from bmc_hip.optim import Adam
    params, gen = _params(dev, [300, 9], 163)
    opt = Adam(params, max_grad_norm=1.0)
    for call in (opt.last_clip, opt.skipped_steps):
        with pytest.raises(RuntimeError, match="before the first step"):
            call()
    off = Adam(params)
    for call in (off.last_clip, off.skipped_steps):
        with pytest.raises(RuntimeError, match="max_grad_norm"):
            call()
    opt.step()                                                # no gradients: nothing is launched, still "before the first step"
    with pytest.raises(RuntimeError, match="before the first step"):
        opt.last_clip()
    opt.max_grad_norm = -1.0                                  # the attribute is checked again at every step
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.step()
    if torch.cuda.device_count() >= 2:
        two = [torch.nn.Parameter(torch.zeros(5, device="cuda:0")), torch.nn.Parameter(torch.zeros(5, device="cuda:1"))]
        opt2 = Adam(two, max_grad_norm=1.0)
        for p in two:
            p.grad = torch.ones_like(p)
        n0 = optim.NORM_LAUNCHES
        with pytest.raises(ValueError, match="one device"):
            opt2.step()
        assert optim.NORM_LAUNCHES == n0 and len(opt2.state) == 0
    # the C ABI: the error code and a message, nothing is launched
    h = optim.step_hyper(1e-3, 0.9, 0.999, 1e-8, 0.0, True, 1.0)
    table = torch.zeros(2 * 48, dtype=torch.uint8, device=dev)
    part = torch.zeros(2, dtype=torch.float64, device=dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)

    def clip(**kw):
        c = lib.AdamClip()
        c.partial_sq, c.n_partials, c.max_norm, c.skip_nonfinite = part.data_ptr(), 2, 1.0, 0
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    for kw, msg in ((dict(n_partials=1), b"n_partials"), (dict(max_norm=0.0), b"max_norm"), (dict(max_norm=float("nan")), b"max_norm"),
                    (dict(max_norm=-1.0), b"max_norm"), (dict(partial_sq=None), b"partial_sq"), (dict(skip_nonfinite=2), b"skip_nonfinite")):
        assert lib._adam_step_clip(table.data_ptr(), 2, h, clip(**kw), None) < 0 and msg in lib.bmc_last_error()
        assert lib._adam_step_clip_cap(table.data_ptr(), 2, h, step_dev.data_ptr(), clip(**kw), None) < 0 and msg in lib.bmc_last_error()
    assert lib._adam_step_clip(None, 2, h, clip(), None) < 0 and b"no chunk table" in lib.bmc_last_error()
    assert lib._adam_step_clip_cap(table.data_ptr(), 2, h, None, clip(), None) < 0 and b"no step counter" in lib.bmc_last_error()
    assert lib._adam_step_clip(None, 0, h, clip(), None) == 0
    assert lib._adam_grad_sq(None, 2, part.data_ptr(), None) < 0 and b"no chunk table" in lib.bmc_last_error()
    assert lib._adam_grad_sq(table.data_ptr(), 2, None, None) < 0 and b"partial_sq" in lib.bmc_last_error()
    assert lib._adam_grad_sq(table.data_ptr(), -1, part.data_ptr(), None) < 0 and b"negative" in lib.bmc_last_error()
    assert lib._adam_grad_sq(None, 0, None, None) == 0
    torch.cuda.synchronize()
    assert int(step_dev.item()) == 0 and float(part.abs().sum()) == 0.0
