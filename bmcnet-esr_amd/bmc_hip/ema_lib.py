"""ctypes binding of include/bmc_hip_ema.h, the companion header of the weight EMA inside the optimizer step (bmc_adam_ema_step and
its three siblings, bmc_ema_swap), from the library's own description of it, bmc_ema_abi(): fn, struct and field records
(lib.bind).  lib.FUNCTIONS, lib.STRUCTS and lib.EXPORTS do not grow."""
from . import lib

FUNCTIONS, STRUCTS, _ = lib.bind("bmc_ema_abi", "this build has no weight EMA in the optimizer step")

AdamEma = lib._mirror("bmc_adam_ema_t", "AdamEma", STRUCTS)          # the entry points below take it by value

_adam_ema_step = lib._sig("bmc_adam_ema_step", FUNCTIONS)
_adam_ema_step_cap = lib._sig("bmc_adam_ema_step_capturable", FUNCTIONS)
_adam_ema_step_clip = lib._sig("bmc_adam_ema_step_clipped", FUNCTIONS)
_adam_ema_step_clip_cap = lib._sig("bmc_adam_ema_step_clipped_capturable", FUNCTIONS)
_ema_swap = lib._sig("bmc_ema_swap", FUNCTIONS)
