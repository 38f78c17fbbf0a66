"""ctypes binding of include/bmc_hip_losses.h, the companion header of the robust-loss head (bmc_head_loss_fwd / _bwd), from the
library's own description of it, bmc_losses_abi(): fn and const records (lib.bind)."""
from . import lib

FUNCTIONS, _, CONSTANTS = lib.bind("bmc_losses_abi", "this build has no robust-loss head")


def const(name):
    """The value of a numeric #define of include/bmc_hip_losses.h."""
    return CONSTANTS[name]


_head_loss_fwd = lib._sig("bmc_head_loss_fwd", FUNCTIONS)
_head_loss_bwd = lib._sig("bmc_head_loss_bwd", FUNCTIONS)
