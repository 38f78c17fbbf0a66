"""ctypes binding of include/bmc_hip_stream.h, the companion header of the continuous (trimmed) event stream
(bmc_slot_emit_trimmed), from the library's own description of it, bmc_stream_abi(): fn, struct, field and const records
(lib.bind)."""
from . import lib

FUNCTIONS, STRUCTS, CONSTANTS = lib.bind("bmc_stream_abi", "this build has no trimmed event output")


def const(name):
    """The value of a numeric #define of include/bmc_hip_stream.h."""
    return CONSTANTS[name]


def dtype(struct):
    """The numpy dtype of a table struct of the header (pointers are <u8), as lib.dtype."""
    return lib.dtype(struct, STRUCTS)


TRIM_PARTS = const("BMC_SLOT_TRIM_PARTS")       # words of `parts` per (slot, part): kept and dropped

_slot_emit_trimmed = lib._sig("bmc_slot_emit_trimmed", FUNCTIONS)
