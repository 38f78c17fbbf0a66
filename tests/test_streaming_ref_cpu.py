"""The float64 restatements of tests/streaming_ref.py against what torch itself computes in float64 (ATen ops + autograd):
float64 on both sides, so agreement is 1e-12 relative.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import streaming_ref as R
from oracle import bmc_oracle

F64 = torch.float64
TOL = 1e-12


def close(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(float(b.abs().max()) if b.numel() else 0.0, 1e-300)
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= TOL * scale, (err, scale)


def rnd(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------ relu_bwd, group_sum, colsum
def test_relu_bwd_selects():
    y = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 3.0, -2.0, float("inf")], dtype=torch.float32)
    dy = torch.arange(1, 8, dtype=torch.float32)
    g = R.relu_bwd(dy, y)
    assert g.dtype == torch.float32 and g.tolist() == [0.0, 0.0, 3.0, 0.0, 5.0, 0.0, 7.0]
    yy = rnd(50).requires_grad_()
    (gg,) = torch.autograd.grad(torch.relu(yy), yy, rnd(50, seed=1))
    close(R.relu_bwd(rnd(50, seed=1), torch.relu(yy).detach()), gg)


@pytest.mark.parametrize("groups", [1, 2, 5])
def test_group_sum(groups):
    x = rnd(groups * 12)
    close(R.group_sum(x, groups), x.view(groups, 12).sum(0))
    x32 = x.float()
    f = R.group_sum_f32(x32, groups)
    assert f.dtype == torch.float32
    if groups == 1:
        assert torch.equal(f, x32)
    if groups == 2:
        assert torch.equal(f, x32[:12] + x32[12:])                      # one rounding: any correct fp32 sum is this one
    # groups - 1 additions, each rounding a partial sum of magnitude <= sum |x|
    bound = (groups - 1) * 2.0 ** -24 * x32.double().abs().view(groups, 12).sum(0)
    assert bool(((f.double() - R.group_sum(x32, groups)).abs() <= bound).all())


@pytest.mark.parametrize("C,stride", [(1, 1), (5, 5), (5, 21), (16, 32)])
def test_colsum(C, stride):
    npix = 17
    buf = rnd(npix * stride + 3)
    want = torch.stack([buf[p * stride:p * stride + C] for p in range(npix)]).sum(0)
    close(R.colsum(buf, npix, stride, C), want)
    prior = rnd(C, seed=2)
    close(R.colsum(buf, npix, stride, C, prior, 1), want + prior)
    close(R.colsum(buf, npix, stride, C, prior, 0), want)


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("C", [4, 48, 100])
def test_layernorm_vs_torch_and_oracle(C):
    npix, eps = 37, 1e-6
    x = (rnd(npix, C) * 2 + 0.5).requires_grad_()
    gamma = (rnd(C, seed=1) + 2).requires_grad_()
    beta = rnd(C, seed=2).requires_grad_()
    dy = rnd(npix, C, seed=3)
    y, stats = R.layernorm_fwd(x, gamma, beta, eps)
    want = F.layer_norm(x, (C,), gamma, beta, eps)
    close(y, want.detach())
    close(stats[:, 0], x.detach().mean(-1))
    close(stats[:, 1], 1 / torch.sqrt(x.detach().var(-1, unbiased=False) + eps))
    gx, gg, gb = torch.autograd.grad(want, (x, gamma, beta), dy)
    dx, dgamma, dbeta = R.layernorm_bwd(dy, x, stats, gamma)
    close(dx, gx), close(dgamma, gg), close(dbeta, gb)
    pg, pb = rnd(C, seed=4), rnd(C, seed=5)
    _, ag, ab = R.layernorm_bwd(dy, x, stats, gamma, pg, pb, 1)
    close(ag, gg + pg), close(ab, gb + pb)
    # the repository's own LayerNorm in float64.  models/submodules.py here has no `LayerNormFunction` class (its LayerNorm2d
    # calls the HIP kernels, fp32 and GPU only), so the plain restatement of that class that the repository keeps stands in for
    # it: oracle/bmc_oracle.py::layer_norm_2d (NCHW), with autograd for the three gradients
    xo = x.detach().view(1, npix, 1, C).permute(0, 3, 1, 2).clone().requires_grad_()
    go, bo = gamma.detach().clone().requires_grad_(), beta.detach().clone().requires_grad_()
    yo = bmc_oracle.layer_norm_2d(xo, go, bo, eps)
    close(y, yo.detach().permute(0, 2, 3, 1).reshape(npix, C))
    ox, og, ob = torch.autograd.grad(yo, (xo, go, bo), dy.view(1, npix, 1, C).permute(0, 3, 1, 2))
    close(dx, ox.permute(0, 2, 3, 1).reshape(npix, C)), close(dgamma, og), close(dbeta, ob)


def test_layernorm_constant_rows():
    x = torch.full((3, 8), 2.5, dtype=F64)
    y, stats = R.layernorm_fwd(x, torch.full((8,), 3.0, dtype=F64), torch.full((8,), -1.0, dtype=F64), 1e-6)
    close(stats[:, 1], torch.full((3,), 1e3, dtype=F64))
    close(y, torch.full((3, 8), -1.0, dtype=F64))


# ------------------------------------------------------------------ softmax
@pytest.mark.parametrize("C", [1, 7, 65])
@pytest.mark.parametrize("scale", [1.0, 128 ** -0.5])
def test_softmax(C, scale):
    a = rnd(5, C) * 3
    a[0, 0], a[1, -1], a[2] = 80.0, -80.0, 1.25
    a.requires_grad_()
    want = torch.softmax(a, -1)
    close(R.softmax_fwd(a), want.detach())
    dp = rnd(5, C, seed=1)
    (ga,) = torch.autograd.grad(want, a, dp)
    close(R.softmax_bwd(want.detach(), dp, scale), ga * scale)


# ------------------------------------------------------------------ pack_inputs
@pytest.mark.parametrize("repeat", [1, 3, 8])
def test_pack_inputs(repeat):
    B, T, H, W = 2, 3, 5, 7
    x = rnd(B, T, H, W, 2).permute(0, 4, 1, 2, 3)[..., ::1]            # a permuted view, T = 3
    f1, f2 = x[:, :, 0, :, :], x[:, :, 1, :, :]                         # models/BMCNet.py:106-112
    parts = [f1[:, 0:1].repeat(1, repeat, 1, 1), f1[:, 1:2].repeat(1, repeat, 1, 1),
             f2[:, 0:1].repeat(1, repeat, 1, 1), f2[:, 1:2].repeat(1, repeat, 1, 1)]
    pad = torch.zeros(B, 16 - 2 * repeat, H, W, dtype=F64)
    want_p = torch.cat([parts[0], parts[2], pad], 1).permute(0, 2, 3, 1)
    want_n = torch.cat([parts[1], parts[3], pad], 1).permute(0, 2, 3, 1)
    xp, xn = R.pack_inputs(x, repeat)
    assert torch.equal(xp, want_p) and torch.equal(xn, want_n)
    poisoned = x.clone()
    poisoned[:, :, 2] = float("nan")                                    # frame 2 is never read
    assert torch.equal(R.pack_inputs(poisoned, repeat)[0], want_p)


# ------------------------------------------------------------------ (un)shuffle, head
@pytest.mark.parametrize("r", [2, 3, 4])
@pytest.mark.parametrize("C,split", [(1, 1), (2, 1), (2, 2)])
def test_shuffle_unshuffle(r, C, split):
    B, H, W = 2, 3, 5
    hr = rnd(B, C, H * r, W * r)
    nchw = F.pixel_unshuffle(hr, r)                                     # [B, C r r, H, W]
    groups = torch.cat(torch.chunk(nchw, split, 1), 0)                  # channel groups along the batch
    want = groups.permute(0, 2, 3, 1)
    lr = R.unshuffle_to_nhwc(hr, r, split)
    assert lr.shape == (split * B, H, W, C * r * r // split) and torch.equal(lr, want)
    back = R.shuffle_to_hr(lr, r, split)
    assert torch.equal(back, hr)
    assert torch.equal(back, F.pixel_shuffle(nchw, r))


@pytest.mark.parametrize("r", [2, 3, 4])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (6, 2)])
def test_head_is_shuffle_plus_bilinear(r, H, W):
    B, C = 2, 2
    lr = rnd(B, H, W, C * r * r)
    frames = rnd(B, 2, 3, H, W, seed=1)
    base = frames[:, :, 1]                                              # a strided slice
    want = F.pixel_shuffle(lr.permute(0, 3, 1, 2), r) + F.interpolate(base, scale_factor=r, mode="bilinear",
                                                                      align_corners=False)
    close(R.shuffle_to_hr(lr, r, 1, base), want)
    up, by, bx = R.bilinear_up(base, r)
    close(up, F.interpolate(base, scale_factor=r, mode="bilinear", align_corners=False))
    assert by.shape == (H * r,) and bx.shape == (W * r,) and bool(by[0]) and bool(by[-1]) and bool(bx[0]) and bool(bx[-1])
    if H >= 3:
        assert not bool(by[r]) and int(by.sum()) == r       # r // 2 rows clamp at 0, (r + 1) // 2 reach the last row


@pytest.mark.parametrize("which", ["dpred", "gloss", "both"])
@pytest.mark.parametrize("r", [2, 4])
def test_head_mse(which, r):
    B, C, H, W = 2, 2, 3, 5
    lr = rnd(B, H, W, C * r * r).requires_grad_()
    base = rnd(B, C, H, W, seed=1)
    gt = rnd(B, C, H * r, W * r, seed=2)
    pred_t = F.pixel_shuffle(lr.permute(0, 3, 1, 2), r) + F.interpolate(base, scale_factor=r, mode="bilinear",
                                                                        align_corners=False)
    loss_t = F.mse_loss(pred_t, gt)
    pred, loss = R.head_mse_fwd(lr, base, gt, r)
    close(pred, pred_t.detach()), close(loss, loss_t.detach())
    dpred = rnd(B, C, H * r, W * r, seed=3) if which != "gloss" else None
    gloss = torch.tensor(0.37, dtype=F64) if which != "dpred" else None
    outs, grads = [], []
    if dpred is not None:
        outs.append(pred_t), grads.append(dpred)
    if gloss is not None:
        outs.append(loss_t), grads.append(gloss)
    (want,) = torch.autograd.grad(outs, lr, grads)
    close(R.head_mse_bwd(dpred, pred, gt, gloss, r), want)


# ------------------------------------------------------------------ bicubic
@pytest.mark.parametrize("H,W,Ho,Wo", [(5, 7, 4, 6), (5, 7, 6, 8), (4, 4, 13, 17), (16, 20, 3, 5), (1, 9, 1, 4), (9, 1, 20, 1),
                                       (31, 56, 62, 111)])
def test_bicubic_matrix(H, W, Ho, Wo):
    P = 2
    x = rnd(P, H, W).requires_grad_()
    want = F.interpolate(x[None], size=(Ho, Wo), mode="bicubic", align_corners=False)[0]
    M = R.bicubic_matrix(H, W, Ho, Wo)
    assert M.shape == (Ho * Wo, H * W)
    close(M.sum(1), torch.ones(Ho * Wo, dtype=F64))                     # every output is an affine combination
    close(R.bicubic_resize_fwd(x, Ho, Wo), want.detach())
    close(R.bicubic_resize_fwd(x, Ho, Wo, dense=False), want.detach())
    gy = rnd(P, Ho, Wo, seed=1)
    (gx,) = torch.autograd.grad(want, x, gy)
    close(R.bicubic_resize_bwd(gy, H, W), gx)
    close(R.bicubic_resize_bwd(gy, H, W, dense=False), gx)


# ------------------------------------------------------------------ chain_affine_grads
@pytest.mark.parametrize("C", [32, 48])
def test_chain_affine_grads(C):
    npx = 23
    yhat, dcentre = rnd(npx, C), rnd(npx, C, seed=1)
    Wc = rnd(C, C, seed=2).requires_grad_()
    bc = rnd(C, seed=3).requires_grad_()
    gamma, beta = (rnd(C, seed=4) + 2).requires_grad_(), rnd(C, seed=5).requires_grad_()
    centre = F.conv2d((yhat * gamma + beta).T.reshape(1, C, npx, 1), Wc.view(C, C, 1, 1), bc)    # clustering(yhat*gamma + beta)
    gw, gbc, gg, gb = torch.autograd.grad(centre, (Wc, bc, gamma, beta), dcentre.T.reshape(1, C, npx, 1))
    G, dbc = dcentre.T @ yhat, dcentre.sum(0)                                                     # what the GEMM hands over
    dwc, dbc_out, dgamma, dbeta = R.chain_affine_grads(G, dbc, Wc, gamma, beta, want_dbc_out=True)
    close(dwc, gw), close(dbc_out, gbc), close(dgamma, gg), close(dbeta, gb)
    assert R.chain_affine_grads(G, dbc, Wc, gamma, beta)[1] is None
    prior = (rnd(C, C, seed=6), rnd(C, seed=7), rnd(C, seed=8), rnd(C, seed=9))
    acc = R.chain_affine_grads(G, dbc, Wc, gamma, beta, prior, 1, True)
    for a, w, p in zip(acc, (gw, gbc, gg, gb), prior):
        close(a, w + p)
