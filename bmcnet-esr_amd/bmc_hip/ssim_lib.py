"""ctypes binding of include/bmc_hip_ssim.h, the companion header of the structural training loss (bmc_ssim_loss_fwd / _bwd),
from the library's own description of it, bmc_ssim_abi(): fn and const records (lib.bind)."""
from . import lib

FUNCTIONS, _, CONSTANTS = lib.bind("bmc_ssim_abi", "this build has no SSIM training loss")


def const(name):
    """The value of a numeric #define of include/bmc_hip_ssim.h."""
    return CONSTANTS[name]


WIN = const("BMC_SSIM_WIN")
TILE_H, TILE_W = const("BMC_SSIM_TILE_H"), const("BMC_SSIM_TILE_W")                    # forward: window positions per workgroup
BWD_TILE_H, BWD_TILE_W = const("BMC_SSIM_BWD_TILE_H"), const("BMC_SSIM_BWD_TILE_W")    # backward: pixels per workgroup
FWD_LAUNCHES, BWD_LAUNCHES = 2, 1


def fwd_tiles(h, w):
    """Tile partials per plane of an h x w image: the doubles of scratch bmc_ssim_loss_fwd needs are B * C times this."""
    return -(-(h - WIN + 1) // TILE_H) * -(-(w - WIN + 1) // TILE_W)


_ssim_loss_fwd = lib._sig("bmc_ssim_loss_fwd", FUNCTIONS)
_ssim_loss_bwd = lib._sig("bmc_ssim_loss_bwd", FUNCTIONS)
