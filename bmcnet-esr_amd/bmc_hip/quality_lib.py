"""ctypes binding of include/bmc_hip_quality.h, the companion header of the slots' PSNR / SSIM (bmc_slot_quality), from the
library's own description of it, bmc_quality_abi(): fn, struct, field and const records (lib.bind)."""
from . import lib

FUNCTIONS, STRUCTS, CONSTANTS = lib.bind("bmc_quality_abi", "this build has no slot quality metrics")


def const(name):
    """The value of a numeric #define of include/bmc_hip_quality.h."""
    return CONSTANTS[name]


def dtype(struct):
    """The numpy dtype of a table struct of the header (pointers are <u8), as lib.dtype."""
    return lib.dtype(struct, STRUCTS)


_slot_quality = lib._sig("bmc_slot_quality", FUNCTIONS)
