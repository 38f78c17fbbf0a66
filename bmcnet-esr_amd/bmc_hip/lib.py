"""ctypes binding of libbmc_hip.so (C ABI: include/bmc_hip.h).

There is no CPU fallback: if the shared library is missing the import of this
module raises, and every call checks the return code and raises RuntimeError
with the library's message.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import numpy as np
import torch  # noqa: F401  -- must come first: libbmc_hip.so has to bind to the HIP runtime torch already loaded
              # (torch ships its own libamdhip64; two runtimes in one process do not share the device context)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BMC_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "libbmc_hip.so")  # override: tools/ experiments only

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build the HIP extension first "
        "(python -c 'import __graft_entry__ as g; g.build()' or make -C bmcnet-esr_amd/csrc). "
        "The BMCNet MI355X path has no CPU fallback.")

_lib = C.CDLL(LIB_PATH)

c_fp = C.c_void_p  # device pointers travel as integers

# ---- the ABI, as the library states it (csrc/abi.hip): nothing below types a signature, an offset or a size by hand ----
Field = namedtuple("Field", "name offset size elem_size code shape")     # code: the element type, i4 / u4 / i8 / f4 / f8, p[:pointee]
Struct = namedtuple("Struct", "size align fields")                       # (a pointer), s:<struct>; shape: array extents; fields: by name


def bind(symbol, lacks):
    """The records of one ABI text of the library, symbol() -- bmc_abi() for include/bmc_hip.h, one per companion header -- as
    (FUNCTIONS, STRUCTS, CONSTANTS): name -> [return code, parameter code, ...] / Struct / int or float.  lacks: what a build
    without the symbol is missing, for the ImportError."""
    try:
        text = getattr(_lib, symbol)
    except AttributeError:
        raise ImportError(f"{LIB_PATH} does not export {symbol}(): {lacks} -- rebuild it") from None
    text.restype, text.argtypes = C.c_char_p, []
    functions, structs, constants = {}, {}, {}
    for kind, name, *rec in (line.split() for line in text().decode().splitlines()):
        if kind == "fn":
            functions[name] = rec
        elif kind == "struct":
            structs[name] = Struct(int(rec[0]), int(rec[1]), {})
        elif kind == "field":
            structs[name].fields[rec[0]] = Field(rec[0], int(rec[1]), int(rec[2]), int(rec[3]), rec[4], tuple(map(int, rec[5:])))
        elif kind == "const":
            constants[name] = (float if rec[0][0] == "f" else int)(rec[1])
        else:
            raise ImportError(f"{LIB_PATH}: unknown record in {symbol}(): {kind} {name}")
    return functions, structs, constants


FUNCTIONS, STRUCTS, CONSTANTS = bind("bmc_abi", "the binding is built from the library's own description of its ABI, and this "
                                     "build (an old one, reached through BMC_HIP_LIB?) has none")
EXPORTS = list(FUNCTIONS) + ["bmc_abi"]


def const(name):
    """The value of a numeric #define of include/bmc_hip.h."""
    return CONSTANTS[name]


def dtype(struct, structs=STRUCTS):
    """The numpy dtype of a table struct of the header (scalar and pointer fields; pointers are <u8).  structs: the table that
    describes it, a companion header's for one of its structs."""
    fields = structs[struct].fields.values()
    return np.dtype({"names": [f.name for f in fields], "offsets": [f.offset for f in fields], "itemsize": structs[struct].size,
                     "formats": [("<u8" if f.code[0] == "p" else "<" + f.code, f.shape) for f in fields]})


_SCALARS = {"i4": C.c_int, "u4": C.c_uint, "i8": C.c_longlong, "f4": C.c_float, "f8": C.c_double, "p": C.c_void_p}
_MIRRORS = {}       # struct name -> its ctypes class


def _ctype(code):
    """Argument / field type of a code: a mirrored struct by value is its class and a pointer to one POINTER(class) (another
    struct passed by byref raises TypeError); every other pointer is c_void_p -- device tables and tensors travel as integers,
    and ctypes arrays / byref() of scalars are accepted as they are."""
    kind, _, name = code.partition(":")
    if kind == "s":
        return _MIRRORS[name]
    if kind == "p":
        return C.POINTER(_MIRRORS[name]) if name in _MIRRORS else C.c_void_p
    return _SCALARS[kind]


def _mirror(struct, cls, structs=STRUCTS):
    """The ctypes mirror of a host struct of the header, fields from the table `structs`.  cls: the new class's name, or a
    Structure subclass that still lacks its _fields_ (one with host-side attributes of its own)."""
    if isinstance(cls, str):
        cls = type(cls, (C.Structure,), {})
    fields = []
    for f in structs[struct].fields.values():
        t = _ctype(f.code)
        for n in reversed(f.shape):
            t = t * n
        fields.append((f.name, t))
    cls._fields_ = fields
    if C.sizeof(cls) != structs[struct].size or any(getattr(cls, f.name).offset != f.offset for f in structs[struct].fields.values()):
        raise ImportError(f"ctypes lays out {struct} differently from the compiler that built {LIB_PATH}")
    _MIRRORS[struct] = cls
    return cls


MAX_SRC = const("BMC_MAX_SRC")
SRC_TABLE = const("BMC_SRC_TABLE")      # Src.batch_mod of an operand whose `ptr` is a device table of per-image base pointers


class Src(C.Structure):
    # Batch segment of a convolution operand (ops.View with a second tensor): launch images b >= seg_b start seg_delta floats
    # past where the descriptor puts image b.  Host-side attributes, NOT part of bmc_src_t: the C ABI carries them at launch
    # level (bmc_conv_args_t::seg_b / *_seg_delta), where ops.conv_raw copies them; every other entry point takes plain operands.
    seg_b = 0
    seg_delta = 0


_mirror("bmc_src_t", Src)
ConvArgs = _mirror("bmc_conv_args_t", "ConvArgs")
PgemmArgs = _mirror("bmc_pgemm_args_t", "PgemmArgs")
ChainFwdArgs = _mirror("bmc_chain_fwd_args_t", "ChainFwdArgs")
ChainBwdArgs = _mirror("bmc_chain_bwd_args_t", "ChainBwdArgs")
MmTerm = _mirror("bmc_mm_term_t", "MmTerm")
SmallMmArgs = _mirror("bmc_small_mm_args_t", "SmallMmArgs")
AdamHyper = _mirror("bmc_adam_hyper_t", "AdamHyper")
AdamClip = _mirror("bmc_adam_clip_t", "AdamClip")


def _sig(name, functions=FUNCTIONS):
    if name not in functions:
        raise ImportError(f"{LIB_PATH}: the library's ABI text does not describe {name} (is it in the function list of csrc/abi.hip?)")
    fn = getattr(_lib, name)
    restype, *params = functions[name]
    fn.argtypes = [_ctype(code) for code in params]
    fn.restype = C.c_char_p if restype == "p:char" else _ctype(restype)
    return fn


bmc_version = _sig("bmc_version")
bmc_last_error = _sig("bmc_last_error")
_events = _sig("bmc_events_to_channels")
_voxel = _sig("bmc_events_to_voxel")
_stack_pol = _sig("bmc_events_to_stack_polarity")
_mask = _sig("bmc_events_to_mask")
_stack = _sig("bmc_events_to_stack")
_enc_raw = _sig("bmc_encode_raw_events")
_events_ws = _sig("bmc_events_binned_ws_bytes")
_events_binned = _sig("bmc_events_to_channels_binned")
_enc_raw_binned = _sig("bmc_encode_raw_events_binned")
_ev_torch_ws = _sig("bmc_events_torch_ws_ints")
_ev_img_torch = _sig("bmc_events_to_image_torch")
_ev_vox_torch = _sig("bmc_events_to_voxel_torch")
_pack_w = _sig("bmc_pack_weight")
_pack_wt = _sig("bmc_pack_weight_t")
_pack_wino = _sig("bmc_pack_weight_wino")
_pack_wino4 = _sig("bmc_pack_weight_wino4")
_ww_nsplit = _sig("bmc_wgrad_wino_nsplit")
_stream_low = _sig("bmc_stream_create_low_priority")
_small_mm = _sig("bmc_small_mm")
_ww = _sig("bmc_wgrad_wino")
_ww_red = _sig("bmc_wgrad_wino_reduce")
_ww_multi = _sig("bmc_wgrad_wino_multi")
_ptr_table = _sig("bmc_ptr_table")
_wino_rows = _sig("bmc_conv_wino_rows")
_ww4_nsplit = _sig("bmc_wgrad_wino4_nsplit")
_ww4 = _sig("bmc_wgrad_wino4")
_ww4_red = _sig("bmc_wgrad_wino4_reduce")
_split_w = _sig("bmc_split_weight")
_conv = _sig("bmc_conv")
_pgemm = _sig("bmc_pgemm")
pgemm_wave_map = _sig("bmc_pgemm_wave_map")
_red_w = _sig("bmc_pgemm_reduce_weight")
_red_wg = _sig("bmc_pgemm_reduce_weight_groups")
_red_p = _sig("bmc_pgemm_reduce_plain")
_colsum = _sig("bmc_colsum")
_relu_bwd = _sig("bmc_relu_bwd")
_ln_fwd = _sig("bmc_layernorm_fwd")
_ln_bwd = _sig("bmc_layernorm_bwd")
_sm_fwd = _sig("bmc_softmax_fwd")
_sm_bwd = _sig("bmc_softmax_bwd")
_pack_in = _sig("bmc_pack_inputs")
_unshuffle = _sig("bmc_unshuffle_to_nhwc")
_shuffle = _sig("bmc_shuffle_to_hr")
_head_mse_fwd = _sig("bmc_head_mse_fwd")
_head_mse_bwd = _sig("bmc_head_mse_bwd")
_group_sum = _sig("bmc_group_sum")
_bicubic_fwd = _sig("bmc_bicubic_resize_fwd")
_bicubic_bwd = _sig("bmc_bicubic_resize_bwd")
_head_resize_mse_fwd = _sig("bmc_head_resize_mse_fwd")
_head_resize_mse_bwd = _sig("bmc_head_resize_mse_bwd")
_chain_fwd = _sig("bmc_chain_fwd")
_chain_bwd = _sig("bmc_chain_bwd")
_chain_affine = _sig("bmc_chain_affine_grads")
_slot_stage = _sig("bmc_slot_stage")
_slot_commit = _sig("bmc_slot_commit")
_slot_metrics = _sig("bmc_slot_metrics")
_slot_encode = _sig("bmc_slot_encode")
_slot_emit = _sig("bmc_slot_emit")
_slot_emit_timed = _sig("bmc_slot_emit_timed")
_slot_emit_clocked = _sig("bmc_slot_emit_clocked")
_slot_emit_timed_ws = _sig("bmc_slot_emit_timed_scratch_bytes")
_slot_hot_update = _sig("bmc_slot_hot_update")
_slot_encode_filtered = _sig("bmc_slot_encode_filtered")
_hot_pixel_mask = _sig("bmc_hot_pixel_mask")
_slot_render = _sig("bmc_slot_render")
_slot_voxel = _sig("bmc_slot_voxel")
_seq_encode = _sig("bmc_seq_encode")
_seq_encode_crop = _sig("bmc_seq_encode_crop")
_adam_step = _sig("bmc_adam_step")
_adam_step_cap = _sig("bmc_adam_step_capturable")
_adam_grad_sq = _sig("bmc_adam_grad_sq")
_adam_step_clip = _sig("bmc_adam_step_clipped")
_adam_step_clip_cap = _sig("bmc_adam_step_clipped_capturable")


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {bmc_last_error().decode()}")


def call(fn, what, *args):
    check(fn(*args), what)


def has_symbol(name: str) -> bool:
    return hasattr(_lib, name)
