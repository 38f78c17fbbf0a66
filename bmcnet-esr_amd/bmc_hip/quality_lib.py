"""ctypes binding of include/bmc_hip_quality.h, the companion header of the slots' PSNR / SSIM (bmc_slot_quality), built like
bmc_hip/lib.py's from the library's own description of it: bmc_quality_abi() (csrc/abi.hip), fn, struct, field and const records."""
import ctypes as C

import numpy as np

from . import lib

try:
    lib._lib.bmc_quality_abi.restype = C.c_char_p
except AttributeError:
    raise ImportError(f"{lib.LIB_PATH} does not export bmc_quality_abi(): this build has no slot quality metrics -- rebuild it") from None
lib._lib.bmc_quality_abi.argtypes = []

FUNCTIONS, STRUCTS, CONSTANTS = {}, {}, {}      # name -> [return code, parameter code, ...] / lib.Struct / int
for _kind, _name, *_rec in (line.split() for line in lib._lib.bmc_quality_abi().decode().splitlines()):
    if _kind == "fn":
        FUNCTIONS[_name] = _rec
    elif _kind == "struct":
        STRUCTS[_name] = lib.Struct(int(_rec[0]), int(_rec[1]), {})
    elif _kind == "field":
        STRUCTS[_name].fields[_rec[0]] = lib.Field(_rec[0], int(_rec[1]), int(_rec[2]), int(_rec[3]), _rec[4], tuple(map(int, _rec[5:])))
    elif _kind == "const":
        CONSTANTS[_name] = (float if _rec[0][0] == "f" else int)(_rec[1])
    else:
        raise ImportError(f"{lib.LIB_PATH}: unknown record in bmc_quality_abi(): {_kind} {_name}")


def const(name):
    """The value of a numeric #define of include/bmc_hip_quality.h."""
    return CONSTANTS[name]


def dtype(struct):
    """The numpy dtype of a table struct of the header (pointers are <u8), as lib.dtype."""
    fields = STRUCTS[struct].fields.values()
    return np.dtype({"names": [f.name for f in fields], "offsets": [f.offset for f in fields], "itemsize": STRUCTS[struct].size,
                     "formats": [("<u8" if f.code[0] == "p" else "<" + f.code, f.shape) for f in fields]})


_slot_quality = lib._sig("bmc_slot_quality", FUNCTIONS)
