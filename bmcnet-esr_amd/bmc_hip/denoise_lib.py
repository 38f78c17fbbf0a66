"""ctypes binding of include/bmc_hip_denoise.h, the companion header of the background-activity noise filter of raw event
columns (bmc_event_denoise), from the library's own description of it, bmc_denoise_abi(): fn and const records (lib.bind)."""
from . import lib

FUNCTIONS, _, CONSTANTS = lib.bind("bmc_denoise_abi", "this build has no event noise filter")


def const(name):
    """The value of a numeric #define of include/bmc_hip_denoise.h."""
    return CONSTANTS[name]


STEP = const("BMC_DENOISE_STEP")                # consecutive events a workgroup takes at a time
LDS_WORDS = const("BMC_DENOISE_LDS_WORDS")      # surface entries a workgroup holds
MAX_W = const("BMC_DENOISE_MAX_W")              # the widest sensor
MAX_SUPPORT = 8
LAUNCHES = 2                                    # bands, finish (the count)

band_rows = lib._sig("bmc_event_denoise_band_rows", FUNCTIONS)          # (H, W) -> rows a workgroup owns, -1: refused
scratch_bytes = lib._sig("bmc_event_denoise_scratch_bytes", FUNCTIONS)  # (H, W) -> bytes of scratch, -1: refused
_event_denoise = lib._sig("bmc_event_denoise", FUNCTIONS)
