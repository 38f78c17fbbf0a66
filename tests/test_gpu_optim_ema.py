"""bmc_hip.optim.Adam(ema_decay=, ema_warmup=) on the MI355X (csrc/optim_ema.hip, csrc/adam_k.h; include/bmc_hip_ema.h).

Two yardsticks.  (1) A twin optimizer WITHOUT the option, fed the same gradients: p and the Adam state must be its bits.  (2) The
numpy float32 restatement of the three EMA lines (tests/optim_ema_ref.py) applied to the device's own new p: the average must be
its bits; and the float64 EMA of the same weights, within the bar that file derives from the roundings.

Tensors are views of NaN-guarded buffers, aligned and packed, the average's layout chosen apart from the parameters'; sizes: those
of tests/test_gpu_optim.py and 255, 256, 257 (one round of the 256 lanes in single elements), 1023, 1024, 1025 (one round of
16-byte vectors), 8193 (two chunks and one element).  The guards are checked after every test that uses them.

Measured (MI355X, test_average_bit_for_bit, printed with -s; the largest error / bar over tensors and the three steps, the same for
all four layouts): 0.000 at decay 0 (flat and warm-up), 0.993 / 0.975 at 0.5 (flat / warm-up), 0.978 / 0.975 at 0.999, 0.971 / 0.975
at 0.9999 -- the bar is a bound, not a typical error: an element whose sum e + s rounds by nearly half an ulp while s is small sits
just under it after one step."""
import numpy as np
import pytest
import torch

import optim_ema_ref as E
import optim_ref as R
from test_gpu_optim import KEYS, SIZES, _bits, _grads, _guarded, _params, _setting_id  # noqa: F401
from test_gpu_optim_clip import Rig
from test_gpu_r2 import _gpu, _restore_math_mode  # noqa: F401

pytestmark = pytest.mark.gpu

ESIZES = SIZES + [255, 256, 257, 1023, 1024, 1025, 8193]
LAYOUTS = pytest.mark.parametrize("aligned,ema_aligned", [(True, True), (True, False), (False, True), (False, False)],
                                  ids=["aligned", "ema_packed", "p_packed", "packed"])
DECAYS = [0.0, 0.5, 0.999, 0.9999]


class EmaRig(Rig):
    """Rig with a sixth guarded buffer, the averages, laid out on its own; they start as copies of the parameters."""

    def __init__(self, dev, aligned, ema_aligned, seed, sizes=ESIZES):
        super().__init__(dev, aligned, seed, sizes)
        self.bufs.append(_guarded(dev, sizes, ema_aligned))
        assert ema_aligned == all(t.data_ptr() % 16 == 0 for t in self.bufs[5][2])
        for e, p in zip(self.bufs[5][2], self.params):
            e.copy_(p.detach())

    def install_state(self, opt, amsgrad):
        super().install_state(opt, amsgrad)
        for i, p in enumerate(self.params):
            opt.state[p]["ema"] = self.bufs[5][2][i]

    def emas(self):
        return [t.detach().cpu().numpy().copy() for t in self.bufs[5][2]]

    def weights(self):
        return [p.detach().cpu().numpy().copy() for p in self.params]


def _cfg(setting, lr=1e-4):
    return dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, **setting)


# ------------------------------------------------------------------ 1. invisible to the rest
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "packed"])
@pytest.mark.parametrize("clip", [{}, dict(max_grad_norm=1e3)], ids=["plain", "clipped"])
@pytest.mark.parametrize("setting", R.SETTINGS, ids=_setting_id)
def test_option_is_invisible_to_parameters_and_state(setting, clip, aligned):
    """Five steps: p, exp_avg, exp_avg_sq and max_exp_avg_sq equal, bit for bit, those of a twin without the option."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    cfg = _cfg(setting)
    rig = EmaRig(dev, aligned, aligned, 201)
    twins = [torch.nn.Parameter(p.detach().clone()) for p in rig.params]
    opt, plain = Adam(rig.params, ema_decay=0.999, ema_warmup=True, **clip, **cfg), Adam(twins, **clip, **cfg)
    rig.install_state(opt, setting["amsgrad"])
    keys = KEYS if setting["amsgrad"] else KEYS[:2]
    for step in range(5):
        grads = _grads(rig.gen, rig.params)
        rig.feed(grads)
        for p, g in zip(twins, grads):
            p.grad = g.clone()
        opt.step(); plain.step()
        for p, q in zip(rig.params, twins):
            assert torch.equal(_bits(p), _bits(q)), step
            assert all(torch.equal(_bits(opt.state[p][k]), _bits(plain.state[q][k])) for k in keys), step
            assert "ema" not in plain.state[q]
    if clip:
        assert torch.equal(opt.last_clip().cpu(), plain.last_clip().cpu()) and float(opt.last_clip()[1]) < 1.0
    assert not any(torch.equal(_bits(e), _bits(p)) for e, p in zip(rig.bufs[5][2][4:], rig.params[4:]))      # (the averages lag)
    assert rig.guards_untouched()


def test_two_optimizers_fed_the_same_gradients_hold_the_same_averages():
    """What several ranks rely on: the step is deterministic, so equal (reduced) gradients give equal averages, bit for bit."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    a, gen = _params(dev, [300, 4097, 9], 203)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oa, ob = (Adam(ps, lr=1e-3, weight_decay=1e-5, amsgrad=True, ema_decay=0.99, max_grad_norm=1.0) for ps in (a, b))
    for _ in range(4):
        grads = _grads(gen, a)
        for ps in (a, b):
            for p, g in zip(ps, grads):
                p.grad = g.clone()
        oa.step(); ob.step()
    for p, q in zip(a, b):
        assert torch.equal(_bits(oa.state[p]["ema"]), _bits(ob.state[q]["ema"])) and torch.equal(_bits(p), _bits(q))
        assert not torch.equal(_bits(oa.state[p]["ema"]), _bits(p))


# ------------------------------------------------------------------ 2. the average, bit for bit
@LAYOUTS
@pytest.mark.parametrize("warmup", [False, True], ids=["flat", "warmup"])
@pytest.mark.parametrize("decay", DECAYS)
def test_average_bit_for_bit(decay, warmup, aligned, ema_aligned):
    """After each of three steps the average equals the float32 restatement applied to the device's own new p and its own
    previous value, and lies within the derived bar of the float64 EMA of the same weights."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    setting = dict(amsgrad=True, weight_decay=1e-5)
    rig = EmaRig(dev, aligned, ema_aligned, 211)
    opt = Adam(rig.params, ema_decay=decay, ema_warmup=warmup, **_cfg(setting, lr=1e-2))
    rig.install_state(opt, True)
    prev = rig.emas()
    refs = [E.Ema64(e) for e in prev]
    worst = 0.0
    for t in (1, 2, 3):
        rig.feed(_grads(rig.gen, rig.params))
        opt.step()
        torch.cuda.synchronize()
        w, now, p_new = E.weight32(decay, warmup, t), rig.emas(), rig.weights()
        for i, (e0, e1, p) in enumerate(zip(prev, now, p_new)):
            assert E.same_bits(e1, E.ema32(e0, p, w)), (t, i, ESIZES[i])
            refs[i].update(p, decay, warmup, t)
            err = np.abs(e1.astype(np.float64) - refs[i].e)
            assert (err <= refs[i].bar).all(), (t, i, float((err / refs[i].bar).max()))
            worst = max(worst, float((err / refs[i].bar).max()))
        prev = now
    print("decay %g warmup %d: worst error / bar %.3f" % (decay, warmup, worst))
    assert [float(opt.state[p]["step"]) for p in rig.params] == [3.0] * len(ESIZES)
    assert rig.guards_untouched()


# ------------------------------------------------------------------ 3. special values
@LAYOUTS
def test_nonfinite_gradients_poison_the_elements_the_restatement_says(aligned, ema_aligned):
    """nonfinite="propagate", unclipped: an Inf and a NaN gradient element make their own p NaN, and with it their own average --
    no other element.  Checked against the restatement and by position."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    rig = EmaRig(dev, aligned, ema_aligned, 223)
    opt = Adam(rig.params, ema_decay=0.5, **_cfg(dict(amsgrad=True, weight_decay=1e-5)))
    rig.install_state(opt, True)
    grads = _grads(rig.gen, rig.params)
    grads[6][4096] = float("inf")                            # the one-by-one tail of the aligned path, the second chunk
    grads[14][8191] = float("nan")                           # the last element of a full chunk's vectors
    grads[9][254] = float("-inf")
    rig.feed(grads)
    prev = rig.emas()
    opt.step()
    torch.cuda.synchronize()
    now, p_new = rig.emas(), rig.weights()
    for i, (e0, e1, p) in enumerate(zip(prev, now, p_new)):
        assert E.same_bits(e1, E.ema32(e0, p, E.weight32(0.5, False, 1))), i
    want = [[] for _ in ESIZES]
    want[6], want[14], want[9] = [4096], [8191], [254]
    assert [np.isnan(e).nonzero()[0].tolist() for e in now] == want == [np.isnan(p).nonzero()[0].tolist() for p in p_new]
    assert rig.guards_untouched()


@LAYOUTS
def test_subnormal_differences_are_kept(aligned, ema_aligned):
    """Zero gradients from a zero state without weight decay leave p as it is (m / den = 0 / eps).  With p = +-2^-130 and the
    average k * 2^-149 away, k = 2 .. 8, d = p - e and s = w * d are subnormal: a kernel that flushed them would leave e where it
    was.  decay 0.5: e moves by k / 2 units of 2^-149, ties to even, as numpy does (k = 1 would round to no move at all)."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    rig = EmaRig(dev, aligned, ema_aligned, 227)
    for i, (p, e) in enumerate(zip(rig.params, rig.bufs[5][2])):
        n = p.numel()
        sign = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0)
        with torch.no_grad():
            p.copy_((sign * 2.0 ** -130).to(dev))
        k = (torch.arange(n) % 7 + 2).to(torch.float64) * 2.0 ** -149
        e.copy_((p.detach().cpu().double() + k).float().to(dev))
    opt = Adam(rig.params, ema_decay=0.5, **_cfg(dict(amsgrad=True, weight_decay=0)))
    rig.install_state(opt, True)
    rig.feed([torch.zeros_like(p) for p in rig.params])
    prev, p_old = rig.emas(), rig.weights()
    assert all((e != p).all() and (np.abs(e.astype(np.float64) - p) <= 8 * 2.0 ** -149).all() for e, p in zip(prev, p_old))
    opt.step()
    torch.cuda.synchronize()
    now, p_new = rig.emas(), rig.weights()
    for i, (e0, e1, p0, p1) in enumerate(zip(prev, now, p_old, p_new)):
        assert np.array_equal(p0.view(np.int32), p1.view(np.int32)), i
        assert E.same_bits(e1, E.ema32(e0, p1, np.float32(0.5))), i
        assert (e1 != e0).all() and (np.abs(e1.astype(np.float64) - p1) < np.abs(e0.astype(np.float64) - p1)).all(), i
    assert rig.guards_untouched()


@LAYOUTS
def test_decay_zero_gives_the_weights_exactly(aligned, ema_aligned):
    """w = 1: e' = e + (p - e).  The parameters have magnitudes in [0.5, 1.5) and an Adam step moves them by a few lr = 1e-3, so p
    and the previous average (the previous p) lie within a factor of two of each other: the difference is exact (Sterbenz) and
    the sum is p.  For unrelated p and e the three lines do NOT give p exactly (e = 1, p = 2^-30: d rounds to -1, e' = 0); what
    holds for every input is the restatement, asserted beside it."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    rig = EmaRig(dev, aligned, ema_aligned, 229)
    for p, e in zip(rig.params, rig.bufs[5][2]):
        r = torch.rand(p.shape, generator=rig.gen)
        with torch.no_grad():
            p.copy_((torch.where(r < 0.5, -1.0, 1.0) * (0.5 + torch.rand(p.shape, generator=rig.gen))).to(dev))
        e.copy_(p.detach())
    opt = Adam(rig.params, ema_decay=0.0, **_cfg(dict(amsgrad=True, weight_decay=1e-5), lr=1e-3))
    rig.install_state(opt, True)
    for step in range(3):
        rig.feed(_grads(rig.gen, rig.params))
        prev = rig.emas()
        opt.step()
        torch.cuda.synchronize()
        for i, (e0, e1, p) in enumerate(zip(prev, rig.emas(), rig.weights())):
            assert E.same_bits(e1, E.ema32(e0, p, np.float32(1.0))), (step, i)
            assert np.array_equal(e1.view(np.int32), p.view(np.int32)) and not np.array_equal(e1, e0), (step, i)
    assert rig.guards_untouched()


# ------------------------------------------------------------------ 4. skip
@LAYOUTS
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_skipped_step_leaves_the_averages_and_counts_for_t(bad, aligned, ema_aligned):
    """nonfinite="skip" and one bad gradient element: all six buffers are bitwise unchanged, guards included, skipped_steps() is 1;
    the next, finite step uses the decay of t = 2 (warm-up: w = 1 - 2 / 11, not 0.9), and p is that of the twin without the option."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    cfg = _cfg(dict(amsgrad=True, weight_decay=1e-5), lr=1e-2)
    rig = EmaRig(dev, aligned, ema_aligned, 233)
    twins = [torch.nn.Parameter(p.detach().clone()) for p in rig.params]
    opt = Adam(rig.params, ema_decay=0.999, ema_warmup=True, max_grad_norm=1e3, nonfinite="skip", **cfg)
    plain = Adam(twins, max_grad_norm=1e3, nonfinite="skip", **cfg)
    rig.install_state(opt, True)
    for e in rig.bufs[5][2]:                                 # averages that are not the weights, between the same guards
        e.add_(torch.randn(e.shape, generator=rig.gen).to(dev) * 1e-2)
    grads = _grads(rig.gen, rig.params)
    grads[7][12292] = bad
    rig.feed(grads)
    for p, g in zip(twins, grads):
        p.grad = g.clone()
    before = rig.snapshot(range(6))
    opt.step(); plain.step()
    assert all(torch.equal(a, b) for a, b in zip(before, rig.snapshot(range(6))))
    assert int(opt.skipped_steps()) == 1 and [float(opt.state[p]["step"]) for p in rig.params] == [1.0] * len(ESIZES)
    grads = _grads(rig.gen, rig.params)
    rig.feed(grads)
    for p, g in zip(twins, grads):
        p.grad = g.clone()
    prev = rig.emas()
    opt.step(); plain.step()
    torch.cuda.synchronize()
    w2 = E.weight32(0.999, True, 2)
    assert float(w2) == float(np.float32(1.0 - 2.0 / 11.0)) != float(E.weight32(0.999, True, 1))
    for i, (e0, e1, p) in enumerate(zip(prev, rig.emas(), rig.weights())):
        assert E.same_bits(e1, E.ema32(e0, p, w2)) and not np.array_equal(e1, e0), i
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(rig.params, twins)) and int(opt.skipped_steps()) == 1
    assert rig.guards_untouched()


# ------------------------------------------------------------------ 5. inside a captured graph
def test_clipped_capturable_step_with_ema_in_a_graph():
    """capturable=True, clipped, nonfinite="skip", EMA with warm-up: one eager step, then [norm, step, advance] captured once and
    replayed four times with new gradients copied into the static .grad buffers, the third replay carrying an Inf -- parameters,
    state and averages bit-identical to the same five steps taken eagerly.  The replays run under sync-debug "error"."""
    dev = _gpu()
    from bmc_hip import optim
    cfg = dict(lr=1e-3, weight_decay=1e-5, amsgrad=True)
    sizes = [5, 4097, 300, 8193]

    def run(graphed):
        params, gen = _params(dev, sizes, 239)
        opt = optim.Adam(params, capturable=True, max_grad_norm=20.0, nonfinite="skip", ema_decay=0.999, ema_warmup=True, **cfg)
        all_grads = [_grads(gen, params, scales=[1e-2, 1.0, 1e-1]) for _ in range(5)]
        all_grads[3][1][4096] = float("inf")
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
        torch.cuda.synchronize()
        if graphed:
            torch.cuda.set_sync_debug_mode("error")
        try:
            for grads in all_grads[1:]:
                for s, g in zip(static, grads):
                    s.copy_(g)
                graph.replay() if graphed else opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        counters = opt.step_counter()
        assert len(counters) == 1 and int(counters[0].item()) == 5 and int(opt.skipped_steps()) == 1
        return [_bits(t) for p in params for t in (p, *(opt.state[p][k] for k in KEYS), opt.state[p]["ema"])], params, opt

    (a, _, _), (b, params, opt) = run(True), run(False)
    assert len(a) == 5 * len(sizes) and all(torch.equal(x, y) for x, y in zip(a, b))
    assert not any(torch.equal(_bits(opt.state[p]["ema"]), _bits(p)) for p in params)


def test_plain_and_capturable_entry_points_give_the_same_average():
    """The host's w (plain) and the device's (capturable, computed from the step counter) are the same bits: three eager steps of
    both, unclipped and with warm-up, where w changes every step."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    a, gen = _params(dev, [300, 4097, 9], 241)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    kw = dict(lr=1e-3, weight_decay=1e-5, amsgrad=True, ema_decay=0.9999, ema_warmup=True)
    oa, ob = Adam(a, **kw), Adam(b, capturable=True, **kw)
    for _ in range(3):
        grads = _grads(gen, a)
        for ps in (a, b):
            for p, g in zip(ps, grads):
                p.grad = g.clone()
        oa.step(); ob.step()
        for p, q in zip(a, b):
            assert torch.equal(_bits(oa.state[p]["ema"]), _bits(ob.state[q]["ema"])) and torch.equal(_bits(p), _bits(q))


# ------------------------------------------------------------------ 6. cohorts and absentees
def test_late_and_absent_parameters():
    """Three parameters: the second gets its first gradient at step 3, the third never.  The late one's average starts from its
    p of that moment and moves with ITS t = 1 (warm-up: w = 0.9) while the first parameter is at t = 3 in the same step(); the
    absent one has no "ema" key and ema_state_dict gives its own value."""
    dev = _gpu()
    from bmc_hip import optim
    params, gen = _params(dev, [300, 4097, 9], 251)
    model = torch.nn.Module()
    model.w = torch.nn.ParameterList(params)
    opt = optim.Adam(params, lr=1e-2, weight_decay=1e-5, amsgrad=True, ema_decay=0.999, ema_warmup=True)
    start = [p.detach().cpu().numpy().copy() for p in params]
    e_first = start[0]
    for step in (1, 2, 3):
        grads = _grads(gen, params, scales=[1e-2, 1.0, 1e-1])
        params[0].grad, params[1].grad, params[2].grad = grads[0], (grads[1] if step == 3 else None), None
        s0 = optim.STEP_LAUNCHES
        opt.step()
        assert optim.STEP_LAUNCHES - s0 == (2 if step == 3 else 1)                         # two step-count cohorts in step 3
        torch.cuda.synchronize()
        e_first = E.ema32(e_first, params[0].detach().cpu().numpy(), E.weight32(0.999, True, step))
        assert E.same_bits(opt.state[params[0]]["ema"].cpu().numpy(), e_first), step
        assert ("ema" in opt.state[params[1]]) == (step == 3)
    assert float(opt.state[params[0]]["step"]) == 3.0 and float(opt.state[params[1]]["step"]) == 1.0
    late = E.ema32(start[1], params[1].detach().cpu().numpy(), E.weight32(0.999, True, 1))
    assert E.same_bits(opt.state[params[1]]["ema"].cpu().numpy(), late)
    assert not np.array_equal(late, params[1].detach().cpu().numpy()) and not np.array_equal(late, start[1])
    assert len(opt.state[params[2]]) == 0 and "ema" not in opt.state[params[2]]
    sd = opt.ema_state_dict(model)
    assert list(sd) == list(model.state_dict()) == ["w.0", "w.1", "w.2"]
    assert torch.equal(_bits(sd["w.0"]), _bits(opt.state[params[0]]["ema"])) and torch.equal(_bits(sd["w.1"]), _bits(opt.state[params[1]]["ema"]))
    assert torch.equal(_bits(sd["w.2"]), _bits(params[2])) and np.array_equal(params[2].detach().cpu().numpy(), start[2])


# ------------------------------------------------------------------ 7. the exchange
@LAYOUTS
def test_swap_exchanges_bitwise_and_is_its_own_inverse(aligned, ema_aligned):
    dev = _gpu()
    from bmc_hip import optim
    rig = EmaRig(dev, aligned, ema_aligned, 257)
    for e in rig.bufs[5][2]:
        e.copy_(torch.randn(e.shape, generator=rig.gen))
    rig.bufs[5][2][3][2] = float("nan"); rig.bufs[5][2][6][4096] = float("-inf")
    with torch.no_grad():
        rig.params[5][7] = -0.0
    opt = optim.Adam(rig.params, ema_decay=0.9, **_cfg(dict(amsgrad=True, weight_decay=0)))
    rig.install_state(opt, True)
    before = rig.snapshot(range(6))
    p0, e0 = [_bits(p) for p in rig.params], [_bits(e) for e in rig.bufs[5][2]]
    v0 = [p._version for p in rig.params]
    s0 = optim.STEP_LAUNCHES
    with opt.ema_weights() as inside:
        assert inside is opt
        v1 = [p._version for p in rig.params]
        assert all(torch.equal(_bits(p), e) for p, e in zip(rig.params, e0))
        assert all(torch.equal(_bits(e), p) for e, p in zip(rig.bufs[5][2], p0))
        mid = rig.snapshot(range(6))
        assert all(torch.equal(a, b) for a, b in zip(before[1:5], mid[1:5])) and not torch.equal(before[0], mid[0])
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            with opt.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            opt.step()
        assert all(torch.equal(a, b) for a, b in zip(mid, rig.snapshot(range(6))))       # the refusals moved nothing
    assert all(torch.equal(a, b) for a, b in zip(before, rig.snapshot(range(6))))         # twice: the identity
    assert all(b > a for a, b in zip(v0, v1)) and all(p._version > b for p, b in zip(rig.params, v1))
    assert optim.STEP_LAUNCHES == s0
    with pytest.raises(KeyError, match="boom"):
        with opt.ema_weights():
            raise KeyError("boom")
    assert all(torch.equal(a, b) for a, b in zip(before, rig.snapshot(range(6))))         # an exception inside still swaps back
    with opt.ema_weights():                                                               # ... and the manager works again
        pass
    assert rig.guards_untouched()


def test_swap_refuses_to_start_during_a_capture_and_without_the_option():
    dev = _gpu()
    from bmc_hip.optim import Adam
    params, gen = _params(dev, [300, 9], 263)
    for p, g in zip(params, _grads(gen, params)):
        p.grad = g
    opt = Adam(params, lr=1e-3, ema_decay=0.9)
    opt.step()
    with opt.ema_weights():                                  # (the exchange's table is on the device before the capture)
        pass
    torch.cuda.synchronize()
    before = [_bits(t) for p in params for t in (p, opt.state[p]["ema"])]
    x = torch.zeros(4, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x.add_(1.0)
        with pytest.raises(RuntimeError, match="graph capture"):
            with opt.ema_weights():
                pass
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, [_bits(t) for p in params for t in (p, opt.state[p]["ema"])]))
    with pytest.raises(RuntimeError, match="needs ema_decay"):
        with Adam(params, lr=1e-3).ema_weights():
            pass


# ------------------------------------------------------------------ 8. the kernels really see the other weights
@pytest.mark.parametrize("plain", [True, False], ids=["BMCNet_plain", "BMCNet"])
def test_forward_inside_the_block_runs_on_the_averages(plain):
    """The models of the golden tests plain_nc16 and bmcnet_nc16 (scale 4, n_c 16, n_b 2; B = 2, 9 x 7 and 10 x 12 frames) after three bptt_steps with
    ema_decay = 0.5: the forward inside ema_weights() equals, bit for bit, the forward of a FRESH model loaded from
    ema_state_dict; the forwards before and after the block equal each other and differ from the one inside.  Every cache between
    a parameter and a kernel (weight packs, chains, ops.bias_dense) is keyed on the parameter's version, which the exchange
    advances."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    from models.BMCNet import BMCNet
    from models.BMCNet_plain import BMCNet_plain
    from train_step import bptt_step
    scale, n_c, n_b, B, L = 4, 16, 2, 2, 3
    H, W = (9, 7) if plain else (10, 12)
    gen = torch.Generator().manual_seed(269)
    inp = torch.poisson(torch.full((B, L, 2, H, W), 0.4), generator=gen).to(dev)
    gt = torch.poisson(torch.full((B, L, 2, scale * H, scale * W), 0.4), generator=gen).to(dev)
    cls = BMCNet_plain if plain else BMCNet

    def forward(m):
        z = lambda c: torch.zeros(B, c, H, W, device=dev)
        x = inp[:, 0:2].transpose(1, 2)
        with torch.no_grad():
            out = m(x, z(n_c), z(2 * scale * scale), True) if plain else m(x, z(n_c), z(n_c), z(n_c), z(2 * scale * scale), True)
            return out[-1].clone()

    torch.manual_seed(271)
    m = cls(scale, n_c, n_b).to(dev)
    opt = Adam(m.parameters(), lr=1e-2, weight_decay=1e-5, amsgrad=True, ema_decay=0.5)
    m.train()
    for _ in range(3):
        bptt_step(m, opt, inp, gt, n_c, scale, plain=plain)
    m.eval()
    before = forward(m)
    with opt.ema_weights():
        inside = forward(m)
    after = forward(m)
    fresh = cls(scale, n_c, n_b).to(dev).eval()
    sd = opt.ema_state_dict(m)
    assert list(sd) == list(m.state_dict())                  # alias keys kept
    fresh.load_state_dict(sd, strict=True)
    assert torch.equal(_bits(inside), _bits(forward(fresh)))
    assert torch.equal(_bits(before), _bits(after)) and not torch.equal(_bits(before), _bits(inside))
    assert bool(torch.isfinite(inside).all())


# ------------------------------------------------------------------ 9. checkpoints
def test_checkpoint_round_trip_continues_bit_identically_with_the_averages(tmp_path):
    """checkpoint.save_checkpoint / resume (unchanged) carry state[p]["ema"] through state_dict(): the resumed run continues
    bit-identically, averages included."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    from checkpoint import resume, save_checkpoint

    def toy():
        torch.manual_seed(0)
        m = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3)).to(dev)
        return m, Adam(m.parameters(), lr=1e-2, weight_decay=1e-5, amsgrad=True, ema_decay=0.9, ema_warmup=True)

    def train(m, opt, steps, seed):
        g = torch.Generator().manual_seed(seed)
        for _ in range(steps):
            x = torch.randn(4, 6, generator=g).to(dev)
            opt.zero_grad()
            m(x).pow(2).mean().backward()
            opt.step()

    m, opt = toy()
    train(m, opt, 4, seed=1)
    path = str(tmp_path / "checkpoint-iteration4.pth")
    save_checkpoint(path, m, opt, None, iteration=4)
    saved = [opt.state[p]["ema"].clone() for p in m.parameters()]
    train(m, opt, 3, seed=2)
    m2, opt2 = toy()
    assert resume(path, m2, opt2)["iteration"] == 4
    assert all(torch.equal(opt2.state[p]["ema"], e) and opt2.state[p]["ema"].is_cuda for p, e in zip(m2.parameters(), saved))
    train(m2, opt2, 3, seed=2)
    for a, b in zip(m.parameters(), m2.parameters()):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(opt.state[a]["ema"]), _bits(opt2.state[b]["ema"]))
        assert all(torch.equal(opt.state[a][k], opt2.state[b][k]) for k in KEYS) and float(opt2.state[b]["step"]) == 7.0
        assert not torch.equal(opt.state[a]["ema"], a)


def test_state_dicts_interchange_with_torch_adam():
    """A torch.optim.Adam state dict (no "ema" key) loads, and the averages start from the weights as they are at the next step;
    our state dict loads into torch.optim.Adam on the GPU, which steps and carries the key along."""
    dev = _gpu()
    from bmc_hip.optim import Adam
    cfg = dict(lr=1e-2, weight_decay=1e-5, amsgrad=True)
    params, gen = _params(dev, [300, 4097], 277)
    feed = lambda: [setattr(p, "grad", g) for p, g in zip(params, _grads(gen, params))]
    yard = torch.optim.Adam(params, foreach=False, **cfg)
    feed(); yard.step()
    ours = Adam(params, ema_decay=0.5, **cfg)
    ours.load_state_dict(yard.state_dict())
    assert not any("ema" in ours.state[p] for p in params)
    now = [p.detach().cpu().numpy().copy() for p in params]
    feed(); ours.step()
    torch.cuda.synchronize()
    for p, p0 in zip(params, now):                           # started from the weights of that moment, moved with t = 2
        assert float(ours.state[p]["step"]) == 2.0
        assert E.same_bits(ours.state[p]["ema"].cpu().numpy(), E.ema32(p0, p.detach().cpu().numpy(), E.weight32(0.5, False, 2)))
    sd = ours.state_dict()
    assert sorted(sd["state"][0]) == ["ema", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "step"]
    assert not any("ema" in k for g in sd["param_groups"] for k in g)
    back = torch.optim.Adam(params, foreach=False, **cfg)
    back.load_state_dict(sd)
    kept = [back.state[p]["ema"].clone() for p in params]
    feed(); back.step()
    assert all(torch.equal(back.state[p]["ema"], e) and e.is_cuda for p, e in zip(params, kept))
    assert [float(back.state[p]["step"]) for p in params] == [3.0, 3.0] and all(bool(torch.isfinite(p).all()) for p in params)


# ------------------------------------------------------------------ 10. no host round trip
@pytest.mark.parametrize("clip", [{}, dict(max_grad_norm=1.0, nonfinite="skip")], ids=["plain", "clipped"])
def test_steps_with_the_option_make_no_host_round_trip(clip):
    """Ten steps under torch.cuda.set_sync_debug_mode("error") after the first; one chunk table is copied in all, and the step
    launches are counted as without the option: no launch is added."""
    dev = _gpu()
    from bmc_hip import optim
    counts = {}
    for ema in (dict(ema_decay=0.999, ema_warmup=True), {}):
        params, gen = _params(dev, [300, 4097, 9], 281)
        opt = optim.Adam(params, lr=1e-3, weight_decay=1e-5, amsgrad=True, **clip, **ema)
        for p, g in zip(params, _grads(gen, params)):
            p.grad = g
        c0, s0, n0 = optim.TABLE_COPIES, optim.STEP_LAUNCHES, optim.NORM_LAUNCHES
        opt.step()
        torch.cuda.synchronize()
        probe = torch.ones(1, device=dev)
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                probe.item()
            for _ in range(10):
                opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        counts[bool(ema)] = (optim.TABLE_COPIES - c0, optim.STEP_LAUNCHES - s0, optim.NORM_LAUNCHES - n0)
        if ema:
            assert not any(torch.equal(opt.state[p]["ema"], p) for p in params)
    assert counts[True] == counts[False] == (1, 11, 11 if clip else 0)


# ------------------------------------------------------------------ 11. the C ABI's refusals
def test_c_abi_refusals():
    """NULL EMA array with chunks, decay 1.0 / NaN / negative and a bad flag: -1 and a message from each of the four entry points,
    nothing is launched (the table is all zeros: a launch would fault on its NULL pointers; the counter and the partials stay)."""
    dev = _gpu()
    from bmc_hip import ema_lib, lib, optim
    h = optim.step_hyper(1e-3, 0.9, 0.999, 1e-8, 0.0, True, 1.0)
    table = torch.zeros(2 * 48, dtype=torch.uint8, device=dev)
    eptr = torch.zeros(2, dtype=torch.int64, device=dev)
    part = torch.zeros(2, dtype=torch.float64, device=dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    clip = lib.AdamClip()
    clip.partial_sq, clip.n_partials, clip.max_norm, clip.skip_nonfinite = part.data_ptr(), 2, 1.0, 0

    def ema(**kw):
        e = ema_lib.AdamEma()
        e.e, e.decay, e.w, e.warmup = eptr.data_ptr(), 0.9, 0.1, 0
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    t = table.data_ptr()
    calls = {
        "bmc_adam_ema_step": lambda n, e: ema_lib._adam_ema_step(t, n, h, e, None, None),
        "bmc_adam_ema_step_capturable": lambda n, e: ema_lib._adam_ema_step_cap(t, n, h, e, step_dev.data_ptr(), None, None),
        "bmc_adam_ema_step_clipped": lambda n, e: ema_lib._adam_ema_step_clip(t, n, h, e, clip, None),
        "bmc_adam_ema_step_clipped_capturable": lambda n, e: ema_lib._adam_ema_step_clip_cap(t, n, h, e, step_dev.data_ptr(), clip, None),
    }
    for name, call in calls.items():
        for kw, msg in ((dict(e=None), b"no EMA pointer array"), (dict(decay=1.0), b"decay"), (dict(decay=float("nan")), b"decay"),
                        (dict(decay=-0.1), b"decay"), (dict(decay=float("inf")), b"decay"), (dict(warmup=2), b"warmup"),
                        (dict(warmup=-1), b"warmup")):
            assert call(2, ema(**kw)) == -1, (name, kw)
            assert msg in lib.bmc_last_error() and name.encode() + b":" in lib.bmc_last_error(), (name, kw, lib.bmc_last_error())
        assert call(0, ema(e=None)) == 0                      # no chunks: nothing to point at, nothing launched
        assert call(-1, ema()) == -1 and b"negative" in lib.bmc_last_error()
    assert ema_lib._adam_ema_step(t, 2, h, ema(w=float("nan")), None, None) == -1 and b"not finite" in lib.bmc_last_error()
    assert ema_lib._adam_ema_step(None, 2, h, ema(), None, None) == -1 and b"no chunk table" in lib.bmc_last_error()
    assert ema_lib._adam_ema_step_cap(t, 2, h, ema(), None, None, None) == -1 and b"no step counter" in lib.bmc_last_error()
    assert ema_lib._ema_swap(None, eptr.data_ptr(), 2, None) == -1 and b"no chunk table" in lib.bmc_last_error()
    assert ema_lib._ema_swap(t, None, 2, None) == -1 and b"no EMA pointer array" in lib.bmc_last_error()
    assert ema_lib._ema_swap(t, eptr.data_ptr(), -1, None) == -1 and b"negative" in lib.bmc_last_error()
    assert ema_lib._ema_swap(None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert int(step_dev.item()) == 0 and float(part.abs().sum()) == 0.0
