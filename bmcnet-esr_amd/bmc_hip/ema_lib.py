"""ctypes binding of include/bmc_hip_ema.h, the companion header of the weight EMA inside the optimizer step (bmc_adam_ema_step and
its three siblings, bmc_ema_swap), built like bmc_hip/lib.py's from the library's own description of it: bmc_ema_abi()
(csrc/abi.hip), fn, struct and field records.  lib.FUNCTIONS, lib.STRUCTS and lib.EXPORTS do not grow."""
import ctypes as C

from . import lib

try:
    lib._lib.bmc_ema_abi.restype = C.c_char_p
except AttributeError:
    raise ImportError(f"{lib.LIB_PATH} does not export bmc_ema_abi(): this build has no weight EMA in the optimizer step -- rebuild it") from None
lib._lib.bmc_ema_abi.argtypes = []

FUNCTIONS, STRUCTS = {}, {}      # name -> [return code, parameter code, ...] / lib.Struct
for _kind, _name, *_rec in (line.split() for line in lib._lib.bmc_ema_abi().decode().splitlines()):
    if _kind == "fn":
        FUNCTIONS[_name] = _rec
    elif _kind == "struct":
        STRUCTS[_name] = lib.Struct(int(_rec[0]), int(_rec[1]), {})
    elif _kind == "field":
        STRUCTS[_name].fields[_rec[0]] = lib.Field(_rec[0], int(_rec[1]), int(_rec[2]), int(_rec[3]), _rec[4], tuple(map(int, _rec[5:])))
    else:
        raise ImportError(f"{lib.LIB_PATH}: unknown record in bmc_ema_abi(): {_kind} {_name}")


class AdamEma(C.Structure):
    """bmc_adam_ema_t, fields from the table."""


AdamEma._fields_ = [(f.name, lib._ctype(f.code)) for f in STRUCTS["bmc_adam_ema_t"].fields.values()]
if C.sizeof(AdamEma) != STRUCTS["bmc_adam_ema_t"].size or any(getattr(AdamEma, f.name).offset != f.offset
                                                              for f in STRUCTS["bmc_adam_ema_t"].fields.values()):
    raise ImportError(f"ctypes lays out bmc_adam_ema_t differently from the compiler that built {lib.LIB_PATH}")
lib._MIRRORS["bmc_adam_ema_t"] = AdamEma          # the entry points below take it by value

_adam_ema_step = lib._sig("bmc_adam_ema_step", FUNCTIONS)
_adam_ema_step_cap = lib._sig("bmc_adam_ema_step_capturable", FUNCTIONS)
_adam_ema_step_clip = lib._sig("bmc_adam_ema_step_clipped", FUNCTIONS)
_adam_ema_step_clip_cap = lib._sig("bmc_adam_ema_step_clipped_capturable", FUNCTIONS)
_ema_swap = lib._sig("bmc_ema_swap", FUNCTIONS)
