"""Head + bicubic resize + MSE, the parts that need no GPU: tests/head_resize_ref.py (float64: pred, diff, loss, dlr) against
torch's own float64 autograd through pixel_shuffle + bilinear interpolate + bicubic interpolate + mse_loss -- float64 on both
sides, differing only in summation order over a few hundred terms, so agreement is 1e-12 relative; the gather form of the
backward against the dense matrix; the entry points' refusals (they return before anything touches a device); and which path
train_step.bptt_step / valid_step take, seen through a stand-in model on the CPU."""
import pytest
import torch
import torch.nn.functional as F

import head_resize_ref as HR
import streaming_ref as R

F64 = torch.float64
TOL = 1e-12

# (r, C, H, W, gh, gw): the small shapes tests/test_gpu_head_resize.py runs the kernels at, and EventZoom itself
CASES = [(2, 1, 1, 1, 3, 1), (4, 2, 3, 5, 12, 18), (4, 2, 3, 5, 11, 20), (4, 2, 3, 5, 13, 22), (4, 2, 3, 5, 5, 7),
         (4, 2, 31, 56, 124, 222)]


def close(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(float(b.abs().max()), 1e-300)
    err = float((a - b).abs().max())
    assert err <= TOL * scale, (err, scale)


def rnd(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


def _torch_chain(xo, base, gt, r):
    pred = F.pixel_shuffle(xo.permute(0, 3, 1, 2), r) + F.interpolate(base, scale_factor=r, mode="bilinear", align_corners=False)
    sp = F.interpolate(pred, size=gt.shape[-2:], mode="bicubic", align_corners=False)
    return pred, sp, F.mse_loss(sp, gt)


@pytest.mark.parametrize("r,C,H,W,gh,gw", CASES)
def test_ref_vs_torch_float64_autograd(r, C, H, W, gh, gw):
    B = 2
    xo = rnd(B, H, W, C * r * r, seed=1).requires_grad_()
    base, gt = rnd(B, C, H, W, seed=2) * 2, rnd(B, C, gh, gw, seed=3)
    dpred, gloss = rnd(B, C, H * r, W * r, seed=4), torch.tensor(0.37, dtype=F64)
    pred, sp, loss = _torch_chain(xo, base, gt, r)
    rp, rd, rl = HR.fwd(xo, base, gt, r)
    close(rp, pred.detach())
    close(rd, (sp - gt).detach())
    close(rl, loss.detach())
    (g_loss,) = torch.autograd.grad(loss, xo, gloss, retain_graph=True)
    (g_pred,) = torch.autograd.grad(pred, xo, dpred, retain_graph=True)
    close(HR.bwd(None, rd, gloss, r, H * r, W * r), g_loss)
    close(HR.bwd(dpred, None, None, r, H * r, W * r), g_pred)
    close(HR.bwd(dpred, rd, gloss, r, H * r, W * r), g_loss + g_pred)


@pytest.mark.parametrize("r,C,H,W,gh,gw", CASES[:5])
def test_gather_backward_equals_the_dense_matrix(r, C, H, W, gh, gw):
    HH, WW = H * r, W * r
    g = rnd(3, gh, gw, seed=5)
    dense = (g.reshape(3, gh * gw) @ R.bicubic_matrix(HH, WW, gh, gw)).reshape(3, HH, WW)
    close(HR.resize_t_gather(g, HH, WW), dense)
    close(HR.resize_t(g, HH, WW), dense)
    x = rnd(3, HH, WW, seed=6)
    close(HR.resize(x, gh, gw), (x.reshape(3, HH * WW) @ R.bicubic_matrix(HH, WW, gh, gw).T).reshape(3, gh, gw))
    d = rnd(1, 3, gh, gw, seed=7)
    a = HR.bwd(None, d, torch.tensor(1.5), r, HH, WW, gather=True)
    b = HR.bwd(None, d, torch.tensor(1.5), r, HH, WW, gather=False)
    close(a, b)


def test_gather_counts_clamped_taps_once_per_tap():
    """1 input row, 3 output rows: every output row's four taps all fold onto the one input -> weight 1 each (the taps sum to 1)."""
    t = HR._axis_touch(1, 3)
    assert [d for d, _ in t[0]] == [0, 1, 2]
    for _, w in t[0]:
        assert abs(w - 1.0) < 1e-15


# ------------------------------------------------------------------ the entry points refuse before any launch
def test_entry_points_are_exported_and_refuse_bad_arguments():
    from bmc_hip import lib
    for name in ("bmc_head_resize_mse_fwd", "bmc_head_resize_mse_bwd"):
        assert name in lib.EXPORTS and lib.has_symbol(name)
    p = 4096                                                            # never dereferenced: every call below returns at its argument check
    ok_f = [p, 1, 1, 2, 2, 2, p, 4, 4, 2, 1, p, 12, 3, 4, p, p, p, p]

    def fwd(**kw):
        a = list(ok_f)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib._head_resize_mse_fwd(*a, None)

    for i in (0, 6, 11, 15, 17, 18):                                    # xo, base, gt, pred, partials, loss
        assert fwd(**{"a%d" % i: None}) == -1
        assert b"bmc_head_resize_mse_fwd" in lib.bmc_last_error()
    for i in (1, 2, 3, 4, 5, 13, 14):                                   # B, C, H, W, r, gh, gw
        assert fwd(**{"a%d" % i: 0}) == -1
        assert fwd(**{"a%d" % i: -3}) == -1
    bwd = lib._head_resize_mse_bwd
    assert bwd(None, p, None, 1, 1, 2, 2, 2, 3, 4, p, None) == -1      # no gradient at all
    assert bwd(p, None, p, 1, 1, 2, 2, 2, 3, 4, p, None) == -1         # gloss without diff
    assert bwd(p, p, p, 1, 1, 2, 2, 2, 3, 4, None, None) == -1         # no dlr
    assert bwd(p, p, p, 1, 1, 2, 2, 2, 0, 4, p, None) == -1            # gh = 0
    assert b"bmc_head_resize_mse_bwd" in lib.bmc_last_error()


# ------------------------------------------------------------------ which path the steps take
class _StandIn(torch.nn.Module):
    """A plain-model stand-in on the CPU: forward() and forward_loss() in torch, counting their calls."""

    def __init__(self, scale):
        super().__init__()
        self.scale = scale
        self.w = torch.nn.Parameter(torch.tensor(0.5))
        self.calls = {"forward": 0, "forward_loss": 0}
        self.grad_modes, self.train_modes = [], []

    def forward(self, x, h, o, init):
        self.calls["forward"] += 1
        return h, self.w * F.interpolate(x[:, :, 1], scale_factor=self.scale, mode="nearest")

    def forward_loss(self, x, h, o, init, gt):
        self.calls["forward_loss"] += 1
        self.grad_modes.append(torch.is_grad_enabled())
        self.train_modes.append(self.training)
        pred = self.w * F.interpolate(x[:, :, 1], scale_factor=self.scale, mode="nearest")
        sp = pred if pred.shape[-2:] == gt.shape[-2:] else F.interpolate(pred, size=gt.shape[-2:], mode="bicubic",
                                                                          align_corners=False)
        return h, pred, F.mse_loss(sp, gt)


def _stand_in_case():
    torch.manual_seed(0)
    return _StandIn(2), torch.randn(1, 4, 2, 3, 4), torch.randn(1, 4, 2, 5, 9)      # L = 4: 3 windows; gt 5x9 vs prediction 6x8


def test_bptt_step_takes_forward_loss_at_any_gt_size_and_loss_fn_selects_the_unfused_chain(monkeypatch):
    import train_step
    m, inp, gt = _stand_in_case()
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    loss, _ = train_step.bptt_step(m, opt, inp, gt, 3, 2, plain=True)
    assert m.calls == {"forward": 0, "forward_loss": 3}
    g_fused = m.w.grad.clone()
    # a wrapper around F.mse_loss is another object: today's chain (forward + ops.bicubic_resize + loss_fn)
    monkeypatch.setattr(train_step.ops, "bicubic_resize",
                        lambda x, size: F.interpolate(x, size=tuple(size), mode="bicubic", align_corners=False))
    loss2, _ = train_step.bptt_step(m, opt, inp, gt, 3, 2, plain=True, loss_fn=lambda a, b: F.mse_loss(a, b))
    assert m.calls == {"forward": 3, "forward_loss": 3}
    assert torch.allclose(loss, loss2, rtol=1e-6) and torch.allclose(g_fused, m.w.grad, rtol=1e-5)


def test_valid_step_is_forward_only_and_restores_the_mode():
    import train_step
    m, inp, gt = _stand_in_case()
    want = sum(m.forward_loss(inp[:, i:i + 2].transpose(1, 2), None, None, i == 0, gt[:, i + 1])[2] for i in range(3)).detach()
    m.calls["forward_loss"], m.grad_modes, m.train_modes = 0, [], []
    for mode in (True, False):
        m.train(mode)
        loss, mse = train_step.valid_step(m, inp, gt, 3, 2, plain=True)
        assert m.training is mode
        assert not loss.requires_grad and not mse.requires_grad and m.w.grad is None
        assert torch.allclose(loss, want, rtol=1e-6)
    assert m.calls == {"forward": 0, "forward_loss": 6}
    assert m.grad_modes == [False] * 6 and m.train_modes == [False] * 6

    class Boom(_StandIn):
        def forward_loss(self, *a):
            raise ValueError("boom")

    b = Boom(2)
    with pytest.raises(ValueError):
        train_step.valid_step(b, inp, gt, 3, 2, plain=True)
    assert b.training is True                                          # restored on the way out of an error too
