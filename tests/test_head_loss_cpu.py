"""Robust losses on the fused head (L1, Huber, Charbonnier), the parts that need no GPU: tests/head_loss_ref.py (float64: pred, d,
loss, dlr) against torch's own float64 autograd through pixel_shuffle + bilinear interpolate (+ bicubic interpolate where the
ground truth has another size) + F.l1_loss / F.huber_loss / a hand-written Charbonnier -- float64 on both sides, so agreement is
1e-12 relative; the bmc_hip.losses callables against torch's losses and at their special points; the entry points' refusals
(they return before anything touches a device); and which path train_step.bptt_step / valid_step take for which loss object,
seen through a stand-in model on the CPU."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import head_loss_ref as HL
from test_head_resize_cpu import close, rnd

F64 = torch.float64

# (r, C, H, W, gh, gw): sizes that differ (the small shapes of tests/test_gpu_head_loss.py) and sizes that agree
CASES = [(2, 1, 1, 1, 3, 1), (4, 2, 3, 5, 13, 22), (4, 2, 3, 5, 5, 7), (4, 2, 3, 5, 12, 20), (2, 1, 1, 1, 2, 2)]
KINDS = [("l1", 0.0), ("huber", 0.8), ("charbonnier", 1e-3), ("charbonnier", 0.3)]


def _torch_loss(kind, param, a, b):
    if kind == "l1":
        return F.l1_loss(a, b)
    if kind == "huber":
        return F.huber_loss(a, b, delta=param)
    return torch.sqrt((a - b) ** 2 + param ** 2).mean()


@pytest.mark.parametrize("kind,param", KINDS)
@pytest.mark.parametrize("r,C,H,W,gh,gw", CASES)
def test_ref_vs_torch_float64_autograd(r, C, H, W, gh, gw, kind, param):
    B = 2
    xo = rnd(B, H, W, C * r * r, seed=1).requires_grad_()
    base, gt = rnd(B, C, H, W, seed=2) * 2, rnd(B, C, gh, gw, seed=3)
    dpred, gloss = rnd(B, C, H * r, W * r, seed=4), torch.tensor(0.37, dtype=F64)
    pred = F.pixel_shuffle(xo.permute(0, 3, 1, 2), r) + F.interpolate(base, scale_factor=r, mode="bilinear", align_corners=False)
    same = (gh, gw) == (H * r, W * r)
    sp = pred if same else F.interpolate(pred, size=(gh, gw), mode="bicubic", align_corners=False)
    loss = _torch_loss(kind, param, sp, gt)
    rp, rd, rl = HL.fwd(xo, base, gt, r, kind, param)
    close(rp, pred.detach())
    close(rd, (sp - gt).detach())
    close(rl, loss.detach())
    (g_loss,) = torch.autograd.grad(loss, xo, gloss, retain_graph=True)
    (g_pred,) = torch.autograd.grad(pred, xo, dpred, retain_graph=True)
    for gather in (False, True):
        close(HL.bwd(None, rd, gloss, r, H * r, W * r, kind, param, gather), g_loss)
        close(HL.bwd(dpred, None, None, r, H * r, W * r, kind, param, gather), g_pred)
        close(HL.bwd(dpred, rd, gloss, r, H * r, W * r, kind, param, gather), g_loss + g_pred)


def test_ref_pointwise_functions_at_their_special_points():
    d = torch.tensor([0.0, -0.0, 0.5, -0.5, 0.8, -0.8, 2.0, -2.0], dtype=F64)
    assert HL.drho("l1", d, 0.0).tolist() == [0, 0, 1, -1, 1, -1, 1, -1]
    assert HL.rho("huber", d, 0.8).tolist() == [0, 0, 0.125, 0.125, 0.8 * 0.4, 0.8 * 0.4, 0.8 * 1.6, 0.8 * 1.6]
    assert HL.drho("huber", d, 0.8).tolist() == [0, 0, 0.5, -0.5, 0.8, -0.8, 0.8, -0.8]
    assert HL.rho("charbonnier", d[:2], 1e-3).tolist() == [1e-3, 1e-3]
    assert HL.drho("charbonnier", d[:2], 1e-3).tolist() == [0, 0]


# ------------------------------------------------------------------ the callables of bmc_hip.losses
def test_losses_objects_equal_torchs_losses():
    from bmc_hip import loss_lib, losses
    a, b = rnd(3, 2, 7, 5, seed=8) * 2, rnd(3, 2, 7, 5, seed=9)
    for dt, tol in ((F64, 1e-14), (torch.float32, 1e-6)):
        x, y = a.to(dt), b.to(dt)
        for L, want in ((losses.L1(), F.l1_loss(x, y)), (losses.Huber(), F.huber_loss(x, y)),
                        (losses.Huber(0.3), F.huber_loss(x, y, delta=0.3)), (losses.Huber(2.5), F.huber_loss(x, y, delta=2.5)),
                        (losses.Charbonnier(0.1), torch.sqrt((x - y) ** 2 + 0.01).mean())):
            got = L(x, y)
            assert got.dim() == 0 and got.dtype == dt
            assert abs(float(got) - float(want)) <= tol * abs(float(want)), (L, dt)
            xg = x.clone().requires_grad_()                        # and their autograd: torch's own, or the reference's rho'
            (g,) = torch.autograd.grad(L(xg, y), xg)
            ref = HL.drho(L.name, (x - y).to(F64), L.param) / x.numel()
            assert float((g.to(F64) - ref).abs().max()) <= tol, (L, dt)
    assert (losses.L1().kind, losses.Huber().kind, losses.Charbonnier().kind) == (
        loss_lib.const("BMC_LOSS_L1"), loss_lib.const("BMC_LOSS_HUBER"), loss_lib.const("BMC_LOSS_CHARBONNIER"))
    assert (losses.L1().param, losses.Huber().param, losses.Charbonnier().param) == (0.0, 1.0, 1e-3)


def test_losses_objects_at_zero_and_at_delta():
    from bmc_hip import losses
    gt = torch.zeros(1, dtype=F64)
    at = lambda L, v: float(L(torch.tensor([v], dtype=F64), gt))
    assert at(losses.L1(), 0.0) == 0.0 and _grad(losses.L1(), 0.0) == 0.0            # sign(0) = 0
    assert _grad(losses.L1(), 1e-300) == 1.0 and _grad(losses.L1(), -1e-300) == -1.0
    H = losses.Huber(0.75)
    assert at(H, 0.0) == 0.0 and _grad(H, 0.0) == 0.0
    for s in (1.0, -1.0):                                                            # both branches agree at |d| = delta
        assert at(H, s * 0.75) == 0.75 * (0.75 - 0.5 * 0.75) == 0.5 * 0.75 * 0.75
        assert _grad(H, s * 0.75) == s * 0.75
        assert _grad(H, s * 5.0) == s * 0.75 and _grad(H, s * 0.5) == s * 0.5
    Ch = losses.Charbonnier(1e-3)
    assert at(Ch, 0.0) == 1e-3 and _grad(Ch, 0.0) == 0.0
    assert abs(at(Ch, 3.0) - math.sqrt(9.0 + 1e-6)) < 1e-15


def _grad(L, v):
    x = torch.tensor([v], dtype=F64, requires_grad=True)
    (g,) = torch.autograd.grad(L(x, torch.zeros(1, dtype=F64)), x)
    return float(g)


def test_losses_refuse_bad_parameters_and_parse_the_command_line_form():
    from bmc_hip import losses
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            losses.Huber(bad)
        with pytest.raises(ValueError):
            losses.Charbonnier(bad)
    assert losses.parse("mse") is None
    assert isinstance(losses.parse("l1"), losses.L1)
    h, c = losses.parse("huber:0.5"), losses.parse("charbonnier:1e-3")
    assert isinstance(h, losses.Huber) and h.param == 0.5 and isinstance(c, losses.Charbonnier) and c.param == 1e-3
    assert losses.parse("huber").param == 1.0 and losses.parse("charbonnier").param == 1e-3
    for bad in ("l2", "huber:0", "charbonnier:-1", "mse:1", "l1:2", "huber:x"):
        with pytest.raises(ValueError):
            losses.parse(bad)
    assert losses.is_fusable(h) and not losses.is_fusable(F.l1_loss) and not losses.is_fusable(lambda a, b: h(a, b))


# ------------------------------------------------------------------ the companion header and its binding
def test_companion_header_matches_its_abi_text_and_binding():
    """include/bmc_hip_losses.h by the routes tests/test_cabi_and_host.py takes for bmc_hip.h: the header's text (abi_ref's
    regular expressions and classes) and a C compile of it, against bmc_losses_abi() and what bmc_hip/loss_lib.py installs."""
    import ctypes as C
    import re
    import shutil
    import subprocess
    import tempfile
    import abi_ref
    from bmc_hip import lib, loss_lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(abi_ref.INCLUDE, "bmc_hip_losses.h")).read(), flags=re.S)
    declared = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?[a-z][a-z ]*\*?)\s*\b(bmc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, re.M):
        params = [p.strip() for p in params.split(",")]
        declared[name] = [abi_ref.classify(ret)] + ([] if params == ["void"] else [abi_ref.classify(p) for p in params])
    assert sorted(declared) == sorted(loss_lib.FUNCTIONS) == ["bmc_head_loss_bwd", "bmc_head_loss_fwd", "bmc_losses_abi"]
    assert not set(declared) & set(lib.FUNCTIONS)                      # bmc_hip.h's table does not grow
    scalars = {"i4": C.c_int, "i8": C.c_longlong, "f4": C.c_float}
    for name, fn in (("bmc_head_loss_fwd", loss_lib._head_loss_fwd), ("bmc_head_loss_bwd", loss_lib._head_loss_bwd)):
        ret, *params = declared[name]
        assert [c.split(":")[0] for c in loss_lib.FUNCTIONS[name]] == [ret] + params, name
        assert fn.restype is C.c_int and len(fn.argtypes) == len(params), name
        for kind, got in zip(params, fn.argtypes):
            assert got is (C.c_void_p if kind == "p" else scalars[kind]), (name, kind)
    assert [c.split(":")[0] for c in loss_lib.FUNCTIONS["bmc_losses_abi"]] == declared["bmc_losses_abi"] == ["p"]
    names = [n for n in re.findall(r"^#define[ \t]+(BMC_[A-Z0-9_]+)[ \t]+\S", text, re.M)]
    assert sorted(names) == sorted(loss_lib.CONSTANTS) == ["BMC_LOSS_CHARBONNIER", "BMC_LOSS_HUBER", "BMC_LOSS_L1"]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no host C compiler"
    src = '#include <stdio.h>\n#include "bmc_hip_losses.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(
        'printf("%s %%d\\n", (int)(%s));' % (n, n) for n in names)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run([cc, "-I" + abi_ref.INCLUDE, os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    compiled = dict(zip(out[::2], map(int, out[1::2])))
    assert compiled == loss_lib.CONSTANTS and all(type(v) is int for v in loss_lib.CONSTANTS.values())


# ------------------------------------------------------------------ the entry points refuse before any launch
def test_entry_points_are_exported_and_refuse_bad_arguments():
    from bmc_hip import lib, loss_lib
    for name in ("bmc_head_loss_fwd", "bmc_head_loss_bwd"):
        assert name in loss_lib.FUNCTIONS and lib.has_symbol(name)
    L1, HUBER, CHARB = (loss_lib.const("BMC_LOSS_" + k) for k in ("L1", "HUBER", "CHARBONNIER"))
    p = 4096                                                            # never dereferenced: every call below returns at its argument check
    ok_f = [p, 1, 1, 2, 2, 2, p, 4, 4, 2, 1, p, 12, 3, 4, p, p, p, p, HUBER, 1.0]

    def fwd(**kw):
        a = list(ok_f)
        for k, v in kw.items():
            a[int(k[1:])] = v
        rc = loss_lib._head_loss_fwd(*a, None)
        if rc != 0:
            assert b"bmc_head_loss_fwd" in lib.bmc_last_error()
        return rc

    for i in (0, 6, 11, 15, 17, 18):                                    # xo, base, gt, pred, partials, loss
        assert fwd(**{"a%d" % i: None}) == -1
    for i in (1, 2, 3, 4, 5, 13, 14):                                   # B, C, H, W, r, gh, gw
        assert fwd(**{"a%d" % i: 0}) == -1
        assert fwd(**{"a%d" % i: -3}) == -1
    for kind in (0, -1, 4, 99):
        assert fwd(a19=kind) == -1
    for kind in (HUBER, CHARB):
        for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert fwd(a19=kind, a20=bad) == -1
    assert fwd(a3=2 ** 30, a5=2) == -1                                  # rH = 2^31: the prediction is too large
    assert b"too large" in lib.bmc_last_error()
    assert fwd(a4=2 ** 30, a5=2) == -1

    ok_b = [p, p, p, p, 12, p, 1, 1, 2, 2, 2, 3, 4, HUBER, 1.0, p]    # dpred dsave pred gt gsb gloss B C H W r gh gw kind param dlr

    def bwd(**kw):
        a = list(ok_b)
        for k, v in kw.items():
            a[int(k[1:])] = v
        rc = loss_lib._head_loss_bwd(*a, None)
        if rc != 0:
            assert b"bmc_head_loss_bwd" in lib.bmc_last_error()
        return rc

    assert bwd(a0=None, a5=None) == -1                                  # no gradient at all
    assert bwd(a15=None) == -1                                          # no dlr
    assert bwd(a1=None) == -1                                           # gloss without dsave, sizes differ
    assert bwd(a2=None, a11=4, a12=4) == -1                             # gloss without pred, sizes agree
    assert bwd(a3=None, a11=4, a12=4) == -1                             # gloss without gt, sizes agree
    for i in (6, 7, 8, 9, 10, 11, 12):
        assert bwd(**{"a%d" % i: 0}) == -1
    for kind in (0, 4):
        assert bwd(a13=kind) == -1
    for bad in (0.0, float("nan"), float("inf")):
        assert bwd(a14=bad) == -1 and bwd(a13=CHARB, a14=bad) == -1
    assert bwd(a8=2 ** 30) == -1


# ------------------------------------------------------------------ which path the steps take
class _StandIn(torch.nn.Module):
    """A plain-model stand-in on the CPU: forward() and forward_loss() in torch; forward_loss records its loss argument."""

    def __init__(self, scale):
        super().__init__()
        self.scale = scale
        self.w = torch.nn.Parameter(torch.tensor(0.5))
        self.calls = {"forward": 0, "forward_loss": 0}
        self.losses = []

    def _pred(self, x):
        return self.w * F.interpolate(x[:, :, 1], scale_factor=self.scale, mode="nearest")

    def forward(self, x, h, o, init):
        self.calls["forward"] += 1
        return h, self._pred(x)

    def forward_loss(self, x, h, o, init, gt, loss=None):
        self.calls["forward_loss"] += 1
        self.losses.append(loss)
        pred = self._pred(x)
        sp = pred if pred.shape[-2:] == gt.shape[-2:] else F.interpolate(pred, size=gt.shape[-2:], mode="bicubic",
                                                                          align_corners=False)
        return h, pred, (F.mse_loss if loss is None else loss)(sp, gt)


def _stand_in_case(same):
    torch.manual_seed(0)                                                # L = 4: 3 windows; prediction 6x8
    return _StandIn(2), torch.randn(1, 4, 2, 3, 4), torch.randn(1, 4, 2, 6, 8) if same else torch.randn(1, 4, 2, 5, 9)


def _resize_on_cpu(monkeypatch, train_step):
    monkeypatch.setattr(train_step.ops, "bicubic_resize",
                        lambda x, size: x if tuple(x.shape[-2:]) == tuple(size)
                        else F.interpolate(x, size=tuple(size), mode="bicubic", align_corners=False))


@pytest.mark.parametrize("same", [False, True])
@pytest.mark.parametrize("recompute", [False, True])
def test_bptt_step_fuses_a_losses_object_and_nothing_else(same, recompute, monkeypatch):
    import train_step
    from bmc_hip import losses
    _resize_on_cpu(monkeypatch, train_step)
    for L, plain_fn in ((losses.L1(), F.l1_loss), (losses.Huber(0.7), lambda a, b: F.huber_loss(a, b, delta=0.7)),
                        (losses.Charbonnier(0.05), None)):
        m, inp, gt = _stand_in_case(same)
        opt = torch.optim.SGD(m.parameters(), lr=0.0)
        loss, last = train_step.bptt_step(m, opt, inp, gt, 3, 2, plain=True, loss_fn=L, recompute=recompute)
        # checkpointing runs windows 2 and 3 again inside backward
        assert m.calls == {"forward": 0, "forward_loss": 5 if recompute else 3}
        assert all(l is L for l in m.losses)                             # the object itself reaches forward_loss
        g_fused = m.w.grad.clone()
        # a lambda around the same object, and torch's own loss: other callables, the unfused chain
        others = [lambda a, b: L(a, b)] + ([plain_fn] if plain_fn is not None else [])
        for fn in others:
            m.calls, m.losses = {"forward": 0, "forward_loss": 0}, []
            loss2, _ = train_step.bptt_step(m, opt, inp, gt, 3, 2, plain=True, loss_fn=fn, recompute=recompute)
            assert m.calls == {"forward": 5 if recompute else 3, "forward_loss": 0} and m.losses == []
            assert torch.allclose(loss, loss2, rtol=1e-6) and torch.allclose(g_fused, m.w.grad, rtol=1e-5)


def test_bptt_step_mse_passes_no_loss(monkeypatch):
    import train_step
    _resize_on_cpu(monkeypatch, train_step)
    m, inp, gt = _stand_in_case(False)
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    train_step.bptt_step(m, opt, inp, gt, 3, 2, plain=True)
    train_step.bptt_step(m, opt, inp, gt, 3, 2, plain=True, loss_fn=F.mse_loss)
    assert m.calls == {"forward": 0, "forward_loss": 6} and m.losses == [None] * 6
    train_step.bptt_step(m, opt, inp, gt, 3, 2, plain=True, loss_fn=F.l1_loss)
    assert m.calls == {"forward": 3, "forward_loss": 6}


@pytest.mark.parametrize("same", [False, True])
def test_valid_step_routes_like_bptt_step(same, monkeypatch):
    import train_step
    from bmc_hip import losses
    _resize_on_cpu(monkeypatch, train_step)
    m, inp, gt = _stand_in_case(same)
    L = losses.Huber(0.7)
    want = sum(m.forward_loss(inp[:, i:i + 2].transpose(1, 2), None, None, i == 0, gt[:, i + 1], L)[2] for i in range(3)).detach()
    m.calls, m.losses = {"forward": 0, "forward_loss": 0}, []
    for mode in (True, False):
        m.train(mode)
        loss, last = train_step.valid_step(m, inp, gt, 3, 2, plain=True, loss=L)
        assert m.training is mode and not loss.requires_grad and not last.requires_grad and m.w.grad is None
        assert torch.allclose(loss, want, rtol=1e-6)
    assert m.calls == {"forward": 0, "forward_loss": 6} and all(l is L for l in m.losses)
    m.losses = []
    train_step.valid_step(m, inp, gt, 3, 2, plain=True)
    train_step.valid_step(m, inp, gt, 3, 2, plain=True, loss=F.mse_loss)
    assert m.calls == {"forward": 0, "forward_loss": 12} and m.losses == [None] * 6
    for fn in (lambda a, b: L(a, b), lambda a, b: F.huber_loss(a, b, delta=0.7)):
        loss, last = train_step.valid_step(m, inp, gt, 3, 2, plain=True, loss=fn)
        assert torch.allclose(loss, want, rtol=1e-6) and not loss.requires_grad and m.training is False
    assert m.calls == {"forward": 6, "forward_loss": 12}


def test_head_loss_refuses_a_plain_callable():
    from bmc_hip import ops
    x = torch.zeros(1, 1, 1, 4)
    with pytest.raises(TypeError, match="bmc_hip.losses"):
        ops.head_loss(x, torch.zeros(1, 1, 1, 1), torch.zeros(1, 1, 2, 2), 2, F.l1_loss)
