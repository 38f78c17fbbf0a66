"""ctypes binding of include/bmc_hip_downsample.h, the companion header of the integrate-and-fire downsampler of raw event
columns (bmc_event_downsample_keys / _walk / _gather), from the library's own description of it, bmc_downsample_abi(): fn and
const records (lib.bind)."""
from . import lib

FUNCTIONS, _, CONSTANTS = lib.bind("bmc_downsample_abi", "this build has no event downsampler")


def const(name):
    """The value of a numeric #define of include/bmc_hip_downsample.h."""
    return CONSTANTS[name]


MAX_SCALE = const("BMC_DOWNSAMPLE_MAX_SCALE")
MAX_THRESHOLD = const("BMC_DOWNSAMPLE_MAX_THRESHOLD")
LANES = const("BMC_DOWNSAMPLE_LANES")           # events of a keys workgroup, LR pixels of a walk workgroup
TILE = const("BMC_DOWNSAMPLE_TILE")             # events a gather workgroup takes at a time
MAX_PARTS = const("BMC_DOWNSAMPLE_MAX_PARTS")   # the most chunks of a gather launch
LAUNCHES = const("BMC_DOWNSAMPLE_LAUNCHES")     # keys, walk, gather (totals), gather (write)

capacity = lib._sig("bmc_event_downsample_capacity", FUNCTIONS)             # (n, T) -> n // T, -1: refused
chunk = lib._sig("bmc_event_downsample_chunk", FUNCTIONS)                   # (n) -> events of a gather chunk, -1: refused
scratch_bytes = lib._sig("bmc_event_downsample_scratch_bytes", FUNCTIONS)   # (n) -> bytes of scratch, -1: refused
_keys = lib._sig("bmc_event_downsample_keys", FUNCTIONS)
_walk = lib._sig("bmc_event_downsample_walk", FUNCTIONS)
_gather = lib._sig("bmc_event_downsample_gather", FUNCTIONS)
