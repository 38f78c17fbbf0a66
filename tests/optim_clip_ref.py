"""Float64 restatement of the clipped optimizer step (include/bmc_hip.h "optimizer step: clipping") on top of tests/optim_ref.py,
and the float32 coefficient exactly as the kernel rounds it.  CPU only; checked against torch.nn.utils.clip_grad_norm_ followed by
torch.optim.Adam in float64 by tests/test_optim_clip_cpu.py."""
import math

import numpy as np

import optim_ref as R


def global_norm64(grads):
    """L2 norm of all elements of `grads` (float32 arrays or tensors, None left out): squares of float32 values are exact in
    float64, math.fsum adds them without error, one square root."""
    sq = []
    for g in grads:
        if g is not None:
            a = np.asarray(g, dtype=np.float64).reshape(-1)
            sq.append(a * a)
    return math.sqrt(math.fsum(np.concatenate(sq).tolist())) if sq else 0.0


def coeff64(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in float64; a NaN stays NaN (torch.clamp(max=1.0))."""
    with np.errstate(all="ignore"):
        q = np.float64(max_norm) / (np.float64(norm) + np.float64(1e-6))
    return q if np.isnan(q) or q <= 1.0 else np.float64(1.0)


def coeff32(norm, max_norm):
    """The kernel's coefficient from the float64 norm: every line one float32 rounding."""
    f = np.float32
    with np.errstate(all="ignore"):
        n32 = f(norm)
        s = n32 + f(1e-6)
        q = f(max_norm) / s
    assert isinstance(q, np.float32)
    return f(1.0) if q > f(1.0) else q              # a NaN q stays NaN


class ClippedAdam64:
    """R.Adam64 fed g * c, with c the float64 coefficient of the global norm of the step's gradients."""

    def __init__(self, params, max_norm, **cfg):
        self.ref, self.max_norm, self.last = R.Adam64(params, **cfg), max_norm, None

    def step(self, grads, **override):
        norm = global_norm64(grads)
        c = coeff64(norm, self.max_norm)
        self.last = (norm, float(c))
        self.ref.step([None if g is None else np.asarray(g, dtype=np.float64) * c for g in grads], **override)

    def __getattr__(self, name):                    # p, m, v, vmax, steps
        return getattr(self.ref, name)
