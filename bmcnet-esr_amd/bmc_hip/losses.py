"""Robust training losses: L1, Huber, Charbonnier -- callables (pred, gt) -> scalar with mean reduction.

Written in plain torch ops, so they work on any tensor (CPU included) and differentiate through autograd: called like that they
are the unfused chain and the oracle.  An INSTANCE handed to train_step.bptt_step(loss_fn=...) / valid_step(loss=...) or to a
model's forward_loss(..., loss=...) selects the fused head instead (ops.head_loss -> bmc_head_loss_fwd / _bwd), which evaluates
the same rho with `.kind` and `.param`; the definitions are those of include/bmc_hip_losses.h.  Any other callable -- F.l1_loss, a
lambda around one of these objects -- stays on the unfused chain.

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


def is_fusable(loss):
    """True for an instance of one of the classes above: what the fused head can evaluate."""
    return isinstance(loss, (L1, Huber, Charbonnier))


def parse(spec):
    """'mse' -> None (the MSE path), 'l1', 'huber:DELTA', 'charbonnier:EPS' -> the loss object (tools/train_events.py --loss)."""
    name, _, arg = str(spec).partition(":")
    name = name.strip().lower()
    if name in ("mse", "l1"):
        if arg:
            raise ValueError("--loss %s takes no parameter" % name)
        return None if name == "mse" else L1()
    if name in ("huber", "charbonnier"):
        cls = Huber if name == "huber" else Charbonnier
        return cls(float(arg)) if arg else cls()
    raise ValueError("unknown loss %r: mse | l1 | huber:DELTA | charbonnier:EPS" % (spec,))
