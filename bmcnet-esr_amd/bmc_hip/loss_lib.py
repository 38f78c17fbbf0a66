"""ctypes binding of include/bmc_hip_losses.h, the companion header of the robust-loss head (bmc_head_loss_fwd / _bwd), built like
bmc_hip/lib.py's from the library's own description of it: bmc_losses_abi() (csrc/abi.hip), fn and const records."""
import ctypes as C

from . import lib

try:
    lib._lib.bmc_losses_abi.restype = C.c_char_p
except AttributeError:
    raise ImportError(f"{lib.LIB_PATH} does not export bmc_losses_abi(): this build has no robust-loss head -- rebuild it") from None
lib._lib.bmc_losses_abi.argtypes = []

FUNCTIONS, CONSTANTS = {}, {}       # name -> [return code, parameter code, ...] / int
for _kind, _name, *_rec in (line.split() for line in lib._lib.bmc_losses_abi().decode().splitlines()):
    if _kind == "fn":
        FUNCTIONS[_name] = _rec
    elif _kind == "const":
        CONSTANTS[_name] = (float if _rec[0][0] == "f" else int)(_rec[1])
    else:
        raise ImportError(f"{lib.LIB_PATH}: unknown record in bmc_losses_abi(): {_kind} {_name}")


def const(name):
    """The value of a numeric #define of include/bmc_hip_losses.h."""
    return CONSTANTS[name]


_head_loss_fwd = lib._sig("bmc_head_loss_fwd", FUNCTIONS)
_head_loss_bwd = lib._sig("bmc_head_loss_bwd", FUNCTIONS)
