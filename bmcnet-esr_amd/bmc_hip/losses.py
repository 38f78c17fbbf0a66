"""Training losses beyond MSE -- callables (pred, gt) -> scalar: the robust pointwise L1, Huber, Charbonnier (mean reduction), the
structural SSIM (1 - mean SSIM, include/bmc_hip_ssim.h) and Mix, a weighted sum of a pointwise and a structural one.

Written in plain torch ops, so they work on any tensor (CPU included) and differentiate through autograd: called like that they
are the unfused chain and the oracle.  An INSTANCE handed to train_step.bptt_step(loss_fn=...) / valid_step(loss=...) or to a
model's forward_loss(..., loss=...) selects the fused head instead (ops.head_loss -> bmc_head_loss_fwd / _bwd), which evaluates
the same rho with `.kind` and `.param`; the definitions are those of include/bmc_hip_losses.h.  Any other callable -- F.l1_loss, a
lambda around one of these objects -- stays on the unfused chain.  SSIM and Mix instances stay on the library's kernels too: the
prediction of ops.head, ops.bicubic_resize where the sizes differ, ops.ssim_loss (ops.head_structural_loss).

MSE is not here: F.mse_loss (the default) keeps its own fused path."""
import math

import torch

# include/bmc_hip_losses.h's BMC_LOSS_* values (tests/test_head_loss_cpu.py compares them with the library's)
KIND_L1, KIND_HUBER, KIND_CHARBONNIER = 1, 2, 3


class _Loss:
    kind = 0
    name = ""

    def __init__(self, param):
        self.param = float(param)

    def rho(self, d):
        raise NotImplementedError

    def __call__(self, pred, gt):
        return self.rho(pred - gt).mean()

    def __repr__(self):
        return "%s(%g)" % (type(self).__name__, self.param)


def _positive(what, v):
    v = float(v)
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError("%s must be a finite positive number, got %r" % (what, v))
    return v


class L1(_Loss):
    """mean |d|; d/dd = sign(d) with sign(0) = 0."""
    kind = KIND_L1
    name = "l1"

    def __init__(self):
        super().__init__(0.0)

    def rho(self, d):
        return d.abs()

    def __repr__(self):
        return "L1()"


class Huber(_Loss):
    """mean of 0.5 d^2 where |d| < delta, delta (|d| - 0.5 delta) elsewhere (F.huber_loss)."""
    kind = KIND_HUBER
    name = "huber"

    def __init__(self, delta=1.0):
        super().__init__(_positive("Huber: delta", delta))

    def rho(self, d):
        a = d.abs()
        return torch.where(a < self.param, 0.5 * d * d, self.param * (a - 0.5 * self.param))


class Charbonnier(_Loss):
    """mean sqrt(d^2 + eps^2)."""
    kind = KIND_CHARBONNIER
    name = "charbonnier"

    def __init__(self, eps=1e-3):
        super().__init__(_positive("Charbonnier: eps", eps))

    def rho(self, d):
        return torch.sqrt(d * d + self.param * self.param)


class SSIM:
    """1 - mean SSIM over the 7x7 window positions that lie wholly inside the image: uniform window, K1 = 0.01, K2 = 0.03, sample
    covariance, C1 = (K1 R)^2, C2 = (K2 R)^2 with the constant data range R (include/bmc_hip_ssim.h states the contract).

    data_range: the default 1.0 means ONE EVENT -- right for sparse count images, where a window holds a few events at most.
    With dense, large counts pass your own (the largest count you expect, 255 at most): C1 and C2 grow with its square, and a
    range far below the data makes SSIM insensitive to everything but structure in nearly empty windows.

    __call__ is the plain-torch form: float64 internally, the window means through avg_pool2d, the result in pred's dtype; it
    works on the CPU and is the oracle and the unfused chain.  An INSTANCE handed to bptt_step / valid_step / forward_loss
    selects ops.ssim_loss (bmc_ssim_loss_fwd / _bwd) on the prediction of ops.head."""
    kind = "ssim"
    name = "ssim"
    WIN = 7

    def __init__(self, data_range=1.0):
        self.param = _positive("SSIM: data_range", data_range)

    def __call__(self, pred, gt):
        import torch.nn.functional as F
        if pred.dim() != 4 or pred.shape != gt.shape or min(pred.shape[-2:]) < self.WIN:
            raise ValueError("SSIM: pred and gt must be [B, C, h, w] of one shape with h, w >= %d (got %s and %s)"
                             % (self.WIN, tuple(pred.shape), tuple(gt.shape)))
        n = self.WIN * self.WIN
        cn = n / (n - 1.0)
        C1, C2 = (0.01 * self.param) ** 2, (0.03 * self.param) ** 2
        x, y = (t.to(torch.float64).reshape(-1, 1, *t.shape[-2:]) for t in (pred, gt))
        mean = lambda t: F.avg_pool2d(t, self.WIN, 1)
        ux, uy = mean(x), mean(y)
        vx, vy, vxy = cn * (mean(x * x) - ux * ux), cn * (mean(y * y) - uy * uy), cn * (mean(x * y) - ux * uy)
        S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        return (1.0 - S.mean()).to(pred.dtype)

    def __repr__(self):
        return "SSIM(%g)" % self.param


class Mix:
    """(1 - alpha) * pointwise + alpha * structural, 0 < alpha < 1 (0.84: the weight super-resolution work pairs L1 with SSIM at).
    pointwise: None (nn.MSELoss) or an L1 / Huber / Charbonnier object; structural: an SSIM object.  __call__ is the plain-torch
    form of the same value; an INSTANCE as loss_fn / loss keeps the pointwise term on the fused head and adds ops.ssim_loss."""
    kind = "mix"

    def __init__(self, pointwise, structural, alpha=0.84):
        if pointwise is not None and not is_fusable(pointwise):
            raise TypeError("Mix: pointwise must be None (MSE) or an L1 / Huber / Charbonnier object, got %r" % (pointwise,))
        if not isinstance(structural, SSIM):
            raise TypeError("Mix: structural must be an SSIM object, got %r" % (structural,))
        alpha = float(alpha)
        if not (0.0 < alpha < 1.0):
            raise ValueError("Mix: alpha must lie strictly between 0 and 1, got %r" % alpha)
        self.pointwise, self.structural, self.alpha = pointwise, structural, alpha
        self.name = "%s+ssim" % ("mse" if pointwise is None else pointwise.name)

    def __call__(self, pred, gt):
        point = torch.nn.functional.mse_loss(pred, gt) if self.pointwise is None else self.pointwise(pred, gt)
        return (1.0 - self.alpha) * point + self.alpha * self.structural(pred, gt)

    def __repr__(self):
        return "Mix(%r, %r, %g)" % (self.pointwise, self.structural, self.alpha)


def is_fusable(loss):
    """True for an instance of L1 / Huber / Charbonnier: what the fused head can evaluate."""
    return isinstance(loss, (L1, Huber, Charbonnier))


def is_structural(loss):
    """True for an SSIM or Mix instance: what ops.head_structural_loss evaluates."""
    return isinstance(loss, (SSIM, Mix))


def on_device_path(loss):
    """True for every object the training step keeps on the library's kernels (F.mse_loss is recognised by identity there)."""
    return is_fusable(loss) or is_structural(loss)


FORMS = ("mse | l1 | huber:DELTA | charbonnier:EPS | ssim[:R] | POINT+ssim[:R][@ALPHA] with POINT one of mse | l1 | huber[:D] | "
         "charbonnier[:E], e.g. l1+ssim:8@0.84")


def _parse_pointwise(spec, whole):
    name, _, arg = spec.partition(":")
    name = name.strip().lower()
    if name in ("mse", "l1"):
        if arg:
            raise ValueError("--loss %s takes no parameter" % name)
        return None if name == "mse" else L1()
    if name in ("huber", "charbonnier"):
        cls = Huber if name == "huber" else Charbonnier
        return cls(float(arg)) if arg else cls()
    raise ValueError("unknown loss %r: %s" % (whole, FORMS))


def _parse_ssim(spec, whole):
    name, _, arg = spec.partition(":")
    if name.strip().lower() != "ssim":
        raise ValueError("unknown loss %r: %s" % (whole, FORMS))
    return SSIM(float(arg)) if arg else SSIM()


def parse(spec):
    """'mse' -> None (the MSE path), 'l1', 'huber:DELTA', 'charbonnier:EPS', 'ssim[:R]' -> the loss object, and
    'POINT+ssim[:R][@ALPHA]' -> Mix(POINT's object, SSIM(R), ALPHA) (tools/train_events.py --loss)."""
    import re
    whole = str(spec)
    m = re.match(r"^(.*)\+\s*(ssim.*)$", whole, re.I | re.S)      # (a '+' inside a number, huber:1e+3, is not followed by ssim)
    if m is None:
        if whole.strip().lower().startswith("ssim"):
            return _parse_ssim(whole, spec)
        return _parse_pointwise(whole, spec)
    structural, at, alpha = m.group(2).partition("@")
    if at and not alpha.strip():
        raise ValueError("--loss %s: '@' must be followed by the weight ALPHA" % whole)
    args = (float(alpha),) if at else ()
    return Mix(_parse_pointwise(m.group(1), spec), _parse_ssim(structural, spec), *args)
