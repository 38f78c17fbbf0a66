"""Float64 restatement of the optimizer step (include/bmc_hip.h "optimizer step": the six lines, one operation each) and the
error metric of tests/test_gpu_optim.py.  CPU only; checked against oracle.adam_amsgrad_step, tests/golden/adam.npz and
torch.optim.Adam in float64 by tests/test_optim_cpu.py."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_CFG = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, amsgrad=True)     # what wrote golden/adam.npz
SETTINGS = [dict(amsgrad=a, weight_decay=w) for a in (True, False) for w in (0.0, 1e-5)]


def adam_step64(p, g, m, v, vmax, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False):
    """One step, in place, on float64 tensors; `step` is the 1-based count of THIS step."""
    assert all(t.dtype == torch.float64 for t in (p, g, m, v)) and (vmax is None or vmax.dtype == torch.float64)
    beta1, beta2 = betas
    step_size = lr / (1 - beta1 ** step)
    bias_correction2_sqrt = (1 - beta2 ** step) ** 0.5
    if weight_decay != 0:
        g = g + weight_decay * p
    m.copy_(m + (1 - beta1) * (g - m))
    v.copy_(v * beta2 + (1 - beta2) * (g * g))
    if amsgrad:
        vmax.copy_(torch.maximum(vmax, v))
    den = (vmax if amsgrad else v).sqrt() / bias_correction2_sqrt + eps
    p.copy_(p - step_size * (m / den))


class Adam64:
    """The float64 trajectory of a list of tensors: the same interface as the tests need of an optimizer, on the CPU."""

    def __init__(self, params, **cfg):
        self.cfg = cfg
        self.p = [torch.as_tensor(np.asarray(q), dtype=torch.float64).clone() for q in params]
        self.m = [torch.zeros_like(q) for q in self.p]
        self.v = [torch.zeros_like(q) for q in self.p]
        self.vmax = [torch.zeros_like(q) for q in self.p]
        self.steps = [0] * len(self.p)

    def step(self, grads, **override):
        """grads: one float32 tensor / array per parameter, or None (the parameter is skipped and its count stays)."""
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.steps[i] += 1
            adam_step64(self.p[i], torch.as_tensor(np.asarray(g), dtype=torch.float64), self.m[i], self.v[i], self.vmax[i], self.steps[i],
                        **dict(self.cfg, **override))

    def load(self, i, p, m, v, vmax, step):
        """continue from a float32 state (the state-interchange tests)"""
        for dst, src in ((self.p, p), (self.m, m), (self.v, v), (self.vmax, vmax)):
            if src is not None:
                dst[i] = src.detach().double().cpu().clone()
        self.steps[i] = int(step)


def e_state(x, x64):
    """max|x - x64| / max|x64| of one state tensor (0 where the reference is all zero and so is x)"""
    x, x64 = x.detach().double().cpu().reshape(-1), x64.reshape(-1)
    d, s = float((x - x64).abs().max()), float(x64.abs().max())
    return d / s if s > 0 else d


def e_param(p, p64, lr):
    """max|p - p64| / lr of one parameter: the error in units of one step"""
    return float((p.detach().double().cpu().reshape(-1) - p64.reshape(-1)).abs().max()) / lr


def golden():
    return np.load(os.path.join(GOLDEN, "adam.npz"))
