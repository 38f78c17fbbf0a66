"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol include/bmc_hip.h declares, the
drop-in modules keep the reference's state_dict surface, and the host logic (conv channel maps) is consistent."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from bmc_hip import lib
    hdr = open(os.path.join(ROOT, "include", "bmc_hip.h")).read()
    declared = set(re.findall(r"\b(bmc_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 18
    for name in declared:
        assert lib.has_symbol(name), name
    assert set(lib.EXPORTS) == declared
    assert lib.bmc_version() >= 100


# The layout of every struct of the header as it is today: (sizeof, "field code[extents] offset, ...").  Codes as in csrc/abi.hip:
# p a pointer, i4 / u4 / i8 integers, f4 / f8 floats, s:<struct> a struct held by value.  A header edit that moves anything fails
# here and is then made on purpose, with this table.
LAYOUT = {
    "bmc_src_t": (32, "ptr p 0, batch_stride i8 8, pix_stride i4 16, nch i4 20, batch_shift i4 24, batch_mod i4 28"),
    "bmc_conv_args_t": (424, "nsrc i4 0, src s:bmc_src_t[6] 8, wpacked p 200, bias p 208, w_group_stride i8 216, "
                        "bias_group_stride i4 224, batch_per_group i4 228, out p 232, out_batch_stride i8 240, out_pix_stride i4 248, "
                        "B i4 252, H i4 256, W i4 260, Cout i4 264, Coutpad i4 268, taps i4 272, relu i4 276, residual s:bmc_src_t 280, "
                        "mask s:bmc_src_t 312, accumulate i4 344, math i4 348, seg_b i4 352, src_seg_delta i8[6] 360, "
                        "residual_seg_delta i8 408, mask_seg_delta i8 416"),
    "bmc_pgemm_args_t": (296, "a s:bmc_src_t 0, nsrc i4 32, src s:bmc_src_t[6] 40, B i4 232, H i4 236, W i4 240, taps i4 244, "
                         "batch_per_group i4 248, slabs p 256, nsplit i4 264, zeros p 272, bias_slabs p 280, math i4 288, "
                         "tap_groups i4 292"),
    "bmc_chain_fwd_args_t": (152, "s0 s:bmc_src_t 0, s1 s:bmc_src_t 32, wstream p 64, bias_f p 72, bias_c p 80, gamma p 88, beta p 96, "
                             "eps f4 104, yhat p 112, rstd p 120, centre p 128, B i4 136, C i4 140, H i4 144, W i4 148"),
    "bmc_chain_bwd_args_t": (136, "dcentre s:bmc_src_t 0, wstream p 32, gamma p 40, yhat p 48, rstd p 56, dz p 64, ds1 p 72, ds0 p 80, "
                             "ds0_add s:bmc_src_t 88, n i4 120, C i4 124, H i4 128, W i4 132"),
    "bmc_mm_term_t": (96, "a p 0, a_sb i8 8, a_sg i8 16, a_si i4 24, a_sk i4 28, b p 32, b_sb i8 40, b_sg i8 48, b_sk i4 56, "
                      "b_sj i4 60, w p 64, w_sb i8 72, w_sg i8 80, w_sk i4 88"),
    "bmc_small_mm_args_t": (336, "nterms i4 0, t s:bmc_mm_term_t[2] 8, nbatch i4 200, batch_per_group i4 204, M i4 208, N i4 212, "
                            "K i4 216, alpha f4 220, u p 224, u_sb i8 232, u_sg i8 240, v p 248, v_sb i8 256, v_sg i8 264, c p 272, "
                            "c_sb i8 280, c_sg i8 288, c_si i4 296, c_sj i4 300, vec_out p 304, vo_sb i8 312, vo_sg i8 320, "
                            "accumulate i4 328"),
    "bmc_slot_t": (40, "frames p 0, gt p 8, keep p 16, result p 24, flags i4 32, pad_ i4 36"),
    "bmc_slot_events_t": (192, "lr_xs p 0, lr_ys p 8, lr_ps p 16, gt_xs p 24, gt_ys p 32, gt_ps p 40, gt_range i8[2] 48, "
                          "lr_range i8[8][2] 64"),
    "bmc_seq_sample_t": (1112, "lr_xs p 0, lr_ys p 8, lr_ps p 16, gt_xs p 24, gt_ys p 32, gt_ps p 40, noise_xs p 48, noise_ys p 56, "
                         "noise_ps p 64, n_noise i4 72, flips u4 76, paused u4 80, lr_range i8[32][2] 88, gt_range i8[32][2] 600"),
    "bmc_seq_crop_t": (24, "H i4 0, W i4 4, gh i4 8, gw i4 12, top i4 16, left i4 20"),
    "bmc_slot_emit_t": (48, "xs p 0, ys p 8, ps p 16, index_in p 24, index_out p 32, capacity i8 40"),
    "bmc_slot_emit_timed_t": (56, "xs p 0, ys p 8, ps p 16, index_in p 24, index_out p 32, capacity i8 40, ts p 48"),
    "bmc_slot_clock_t": (24, "t_first f8 0, t_last f8 8, ts p 16"),
    "bmc_slot_hot_t": (64, "hot_pixels p 0, hot_mask p 8, first_item i4 16, new_from i4 20, active i4 24, pad_ i4 28, cmin i4[8] 32"),
    "bmc_slot_render_t": (16, "src p 0, dst p 8"),
    "bmc_slot_voxel_t": (8, "dst p 0"),
    "bmc_adam_chunk_t": (48, "p p 0, g p 8, m p 16, v p 24, vmax p 32, n i4 40, aligned i4 44"),
    "bmc_adam_hyper_t": (64, "lr f8 0, beta1_f64 f8 8, beta2_f64 f8 16, beta1 f4 24, one_minus_beta1 f4 28, beta2 f4 32, "
                         "one_minus_beta2 f4 36, eps f4 40, weight_decay f4 44, step_size f4 48, bias_correction2_sqrt f4 52, "
                         "amsgrad i4 56"),
    "bmc_adam_clip_t": (40, "partial_sq p 0, info p 8, skipped p 16, n_partials i4 24, max_norm f4 28, skip_nonfinite i4 32"),
}
MIRRORS = {"bmc_src_t": "Src", "bmc_conv_args_t": "ConvArgs", "bmc_pgemm_args_t": "PgemmArgs", "bmc_chain_fwd_args_t": "ChainFwdArgs",
           "bmc_chain_bwd_args_t": "ChainBwdArgs", "bmc_mm_term_t": "MmTerm", "bmc_small_mm_args_t": "SmallMmArgs",
           "bmc_adam_hyper_t": "AdamHyper", "bmc_adam_clip_t": "AdamClip"}
TABLE_DTYPES = {"bmc_slot_t": "slots.SLOT_DTYPE", "bmc_slot_events_t": "slots.SLOT_EVENTS_DTYPE", "bmc_slot_emit_t": "slots.SLOT_EMIT_DTYPE",
                "bmc_slot_emit_timed_t": "slots.SLOT_EMIT_TIMED_DTYPE", "bmc_slot_clock_t": "slots.SLOT_CLOCK_DTYPE",
                "bmc_slot_hot_t": "slots.SLOT_HOT_DTYPE", "bmc_slot_render_t": "slots.SLOT_RENDER_DTYPE",
                "bmc_slot_voxel_t": "slots.SLOT_VOXEL_DTYPE", "bmc_seq_sample_t": "event_dataset.SEQ_SAMPLE_DTYPE",
                "bmc_seq_crop_t": "event_dataset.SEQ_CROP_DTYPE", "bmc_adam_chunk_t": "optim.CHUNK_DTYPE"}
# Python names that restate a numeric #define of the header
CONSTANT_MIRRORS = {
    "BMC_MAX_SRC": "lib.MAX_SRC", "BMC_SRC_TABLE": "lib.SRC_TABLE", "BMC_CK": "ops.CK", "BMC_MATH_FP32_WINO": "ops.MATH_FP32_WINO",
    "BMC_MATH_FP32_WINO4": "ops.MATH_FP32_WINO4", "BMC_MAX_SLOTS": "slots.MAX_SLOTS", "BMC_SLOT_ACTIVE": "slots.ACTIVE",
    "BMC_SLOT_RESET": "slots.RESET", "BMC_SLOT_MAX_PARTS": "slots.MAX_PARTS", "BMC_SLOT_MAX_SEQN": "slots.MAX_SEQN",
    "BMC_SEQ_MAX_ITEMS": "event_dataset.MAX_ITEMS", "BMC_SLOT_EMIT_MAX_PARTS": "slots.MAX_EMIT_PARTS", "BMC_EVENT_T0": "slots.EVENT_T0",
    "BMC_EVENT_T1": "slots.EVENT_T1", "BMC_SLOT_EMIT_TIMED_MAX_COUNT": "slots.MAX_COUNT_TIMED",
    "BMC_SLOT_EMIT_TIMED_MAX_WINDOW": "slots.MAX_WINDOW_CAPACITY", "BMC_SLOT_RENDER_MAX_PIXELS": "slots.MAX_RENDER_PIXELS",
    "BMC_SLOT_RENDER_MAX_PARTS": "slots.MAX_RENDER_PARTS", "BMC_SLOT_VOXEL_MAX_BINS": "slots.MAX_VOXEL_BINS",
    "BMC_ADAM_CHUNK": "optim.CHUNK"}


def _python_name(path):
    import importlib
    module, name = path.split(".")
    return getattr(importlib.import_module(module if module == "event_dataset" else "bmc_hip." + module), name)


def test_every_struct_layout_matches_header():
    """Every struct of the header four ways: the header's typedefs (its text), a C compile of the header by the host compiler,
    the library's own table (bmc_abi) and what bmc_hip builds from it (ctypes mirrors, numpy table dtypes) -- and all of them
    against the layout frozen in LAYOUT."""
    import ctypes as C
    import abi_ref
    from bmc_hip import lib
    names = abi_ref.struct_names()
    assert len(names) == 20 and sorted(names) == sorted(lib.STRUCTS) == sorted(LAYOUT)
    assert set(MIRRORS) | set(TABLE_DTYPES) == set(names) and not set(MIRRORS) & set(TABLE_DTYPES)
    compiled = abi_ref.compiled_header()[0]
    ctypes_of = {"i4": C.c_int, "u4": C.c_uint, "i8": C.c_longlong, "f4": C.c_float, "f8": C.c_double, "p": C.c_void_p}
    for struct in names:
        table, (c_size, c_fields) = lib.STRUCTS[struct], compiled[struct]
        assert table.size == c_size == LAYOUT[struct][0] and table.size % table.align == 0, struct
        assert list(table.fields) == list(c_fields), struct
        frozen = []
        for f in table.fields.values():
            assert (f.offset, f.size) == c_fields[f.name], (struct, f.name)
            count = 1
            for n in f.shape:
                count *= n
            assert f.size == count * f.elem_size, (struct, f.name)
            if f.code[0] == "s":
                assert f.elem_size == lib.STRUCTS[f.code[2:]].size, (struct, f.name)
            else:
                assert f.elem_size == (8 if f.code[0] == "p" else int(f.code[1:])), (struct, f.name)
            frozen.append("%s %s%s %d" % (f.name, f.code.split(":")[0] if f.code[0] == "p" else f.code,
                                         "".join("[%d]" % n for n in f.shape), f.offset))
        assert ", ".join(frozen) == LAYOUT[struct][1], struct
        if struct in MIRRORS:
            cls = getattr(lib, MIRRORS[struct])
            assert C.sizeof(cls) == c_size and [n for n, _ in cls._fields_] == list(c_fields), struct
            for name, (offset, size) in c_fields.items():
                assert (getattr(cls, name).offset, getattr(cls, name).size) == (offset, size), (struct, name)
            for f in table.fields.values():                  # ... and every field's ctypes type is the one its code names
                t = dict(cls._fields_)[f.name]
                for n in f.shape:
                    assert t._length_ == n, (struct, f.name)
                    t = t._type_
                assert t is (getattr(lib, MIRRORS[f.code[2:]]) if f.code[0] == "s" else ctypes_of[f.code.split(":")[0]]), (struct, f.name)
        else:
            dt = _python_name(TABLE_DTYPES[struct])
            assert dt == lib.dtype(struct) and dt.itemsize == c_size and list(dt.names) == list(c_fields), struct
            for f in table.fields.values():
                sub, offset = dt.fields[f.name]
                assert (offset, sub.itemsize, sub.shape) == (f.offset, f.size, f.shape), (struct, f.name)
                assert sub.base.str == ("<u8" if f.code[0] == "p" else "<" + f.code), (struct, f.name)
    from bmc_hip import encodings
    assert encodings.SEQ_SAMPLE_BYTES == compiled["bmc_seq_sample_t"][0] and encodings.SEQ_CROP_BYTES == compiled["bmc_seq_crop_t"][0]
    assert lib.Src.seg_b == 0 and lib.Src.seg_delta == 0 and "seg_b" not in dict(lib.Src._fields_)      # host-side attributes


def test_signatures_match_header_text():
    """argtypes / restype of every entry point, as bmc_hip/lib.py installed them from the library's table, against the
    declarations cut out of the header's text: the parameter count, the class of every parameter and the return type."""
    import ctypes as C
    import abi_ref
    from bmc_hip import lib
    declared = abi_ref.functions()
    assert set(declared) == set(lib.EXPORTS) == set(lib.FUNCTIONS) | {"bmc_abi"} and len(declared) == 76
    scalars = {"i4": C.c_int, "u4": C.c_uint, "i8": C.c_longlong, "f4": C.c_float, "f8": C.c_double}
    returns = {"bmc_last_error": C.c_char_p, "bmc_abi": C.c_char_p}
    bound = {f.__name__: f for f in vars(lib).values() if isinstance(f, lib._lib._FuncPtr)}
    assert set(bound) == set(lib.FUNCTIONS)                     # every entry point has its alias in lib.py
    bound["bmc_abi"] = lib._lib.bmc_abi
    pointees = {name: {} for name in declared}                  # name -> {parameter index: its installed pointer type}
    for name, (ret, *params) in declared.items():
        fn = bound[name]
        assert fn.restype is (returns[name] if ret == "p" else scalars[ret]), name
        assert len(fn.argtypes) == len(params), name
        for i, (kind, got) in enumerate(zip(params, fn.argtypes)):
            if kind == "p":
                assert got is C.c_void_p or (issubclass(got, C._Pointer) and got._type_ in [getattr(lib, m) for m in MIRRORS.values()]), (name, i)
                pointees[name][i] = got
            elif kind in scalars:
                assert got is scalars[kind], (name, i)
            else:
                assert got is getattr(lib, MIRRORS[kind]), (name, i)
    # a pointer to a mirrored struct is POINTER(its class): another struct passed by byref is a TypeError, not a launch
    assert pointees["bmc_conv"][0] is C.POINTER(lib.ConvArgs) and pointees["bmc_pgemm"][0] is C.POINTER(lib.PgemmArgs)
    assert pointees["bmc_wgrad_wino"][0] is pointees["bmc_wgrad_wino"][1] is C.POINTER(lib.Src)
    assert pointees["bmc_small_mm"][0] is C.POINTER(lib.SmallMmArgs) and pointees["bmc_chain_fwd"][0] is C.POINTER(lib.ChainFwdArgs)
    assert pointees["bmc_chain_bwd"][0] is C.POINTER(lib.ChainBwdArgs)
    with pytest.raises(C.ArgumentError):
        lib._conv(C.byref(lib.PgemmArgs()), None)
    with pytest.raises(C.ArgumentError):
        lib._adam_step(None, 0, lib.AdamClip(), None, None)


def test_constants_match_header():
    """The numeric #defines: the header's text names exactly the table's; a C compile of the header gives the table's values;
    every Python name that restates one has that value."""
    import abi_ref
    from bmc_hip import lib, ops
    names = abi_ref.constant_names()
    assert len(names) == 24 and sorted(names) == sorted(lib.CONSTANTS)
    compiled = abi_ref.compiled_header()[1]
    for name in names:
        assert lib.const(name) == compiled[name], name
        assert isinstance(lib.const(name), float if name in ("BMC_EVENT_T0", "BMC_EVENT_T1") else int), name
    for name, path in CONSTANT_MIRRORS.items():
        value = _python_name(path)
        assert value == lib.const(name) and type(value) is type(lib.const(name)), name
    assert ops.MATH_NAMES == {"fp32": lib.const("BMC_MATH_FP32"), "bf16": lib.const("BMC_MATH_BF16"), "bf16x6": lib.const("BMC_MATH_BF16X6")}
    assert (lib.MAX_SRC, ops.CK, lib.SRC_TABLE, ops.MATH_NAMES, ops.MATH_FP32_WINO, ops.MATH_FP32_WINO4) == \
        (6, 16, -1, {"fp32": 0, "bf16": 1, "bf16x6": 3}, 4, 5)


def test_state_dict_surface_matches_reference_counts():
    from models.BMCNet import BMCNet
    from models.BMCNet_plain import BMCNet_plain
    m = BMCNet(4, 128, 5)
    assert len(m.state_dict()) == 318 and len(list(m.parameters())) == 54
    assert sum(p.numel() for p in m.parameters()) == 2731680
    p = BMCNet_plain(4, 128, 5)
    assert len(p.state_dict()) == 120 and len(list(p.parameters())) == 24
    assert sum(q.numel() for q in p.parameters()) == 1003296
    sd = m.state_dict()
    assert sd["neuro.conv_fnst.weight"].data_ptr() == sd["neuro.conv_fpst.weight"].data_ptr()
    assert sd["neuro.para_reschunk.4.lBIE.conv2.conv1.weight"].data_ptr() == sd["neuro.para_reschunk.0.lBIE.conv1.conv1.weight"].data_ptr()
    assert sd["neuro.para_reschunk.0.gBIE.convf2.weight"].data_ptr() == sd["neuro.para_reschunk.0.gBIE.convf1.weight"].data_ptr()


def test_state_dict_keys_equal_golden_reference_keys():
    import numpy as np
    from models.BMCNet import BMCNet
    from models.BMCNet_plain import BMCNet_plain
    g = os.path.join(ROOT, "tests", "golden")
    for tag, cls in (("bmcnet_nc16", BMCNet), ("plain_nc16", BMCNet_plain)):
        z = np.load(os.path.join(g, tag + ".npz"))
        ref_keys = sorted(k[3:] for k in z.files if k.startswith("sd/"))
        scale, n_c, n_b = (int(v) for v in z["meta"][:3])
        assert sorted(cls(scale, n_c, n_b).state_dict().keys()) == ref_keys


def test_pretrained_plain_checkpoint_loads_strictly(tmp_path):
    from pretrained_checkpoint import write_reference_checkpoint
    ck = write_reference_checkpoint(str(tmp_path / "BMCNet_plain_nfs_x4.pth"))
    from models.BMCNet_plain import BMCNet_plain
    m = BMCNet_plain(4, 128, 5)
    assert not any(m.load_state_dict(torch.load(ck, map_location="cpu"), strict=True))


def test_conv_specs_cover_every_reference_input_channel_once():
    from models.BMCNet import BMCNet
    from models.BMCNet_plain import BMCNet_plain
    for m in (BMCNet(4, 32, 1).neuro, BMCNet_plain(4, 32, 1).neuro):
        for name, spec in vars(m).items():
            if not name.startswith("_sp_"):
                continue
            used = sorted(c for c in spec.kmap_host if c >= 0)
            assert spec.kpad % 16 == 0 and spec.kreal == len(used)
            if spec.covers_all:
                assert used == list(range(spec.cin)), name
            else:       # one launch of a convolution evaluated as several launches over column subsets of ONE parameter
                assert name in ("_sp_fs_shared", "_sp_fs_h") and len(set(used)) == len(used) < spec.cin
    b = BMCNet(4, 32, 1).neuro
    assert b._sp_fpst.cin == b.conv_fpst.in_channels and b._sp_fps.cin == b.conv_fps.in_channels
    assert b._sp_o.cin == b.conv_o.in_channels
    # conv_fs: the shared launch and the per-state launch name disjoint columns that together are all of conv_fs.weight's
    both = sorted(c for sp in (b._sp_fs_shared, b._sp_fs_h) for c in sp.kmap_host if c >= 0)
    assert b._sp_fs_shared.cin == b._sp_fs_h.cin == b.conv_fs.in_channels and both == list(range(b.conv_fs.in_channels))
    p = BMCNet_plain(4, 32, 1).neuro
    assert p._sp_f1.cin == p.conv_f1.in_channels and p._sp_fs.cin == p.conv_fs.in_channels


def test_no_cpu_fallback():
    from models.BMCNet_plain import BMCNet_plain
    m = BMCNet_plain(4, 16, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 2, 2, 4, 4), torch.zeros(1, 16, 4, 4), torch.zeros(1, 32, 4, 4), True)
    from bmc_hip.encodings import events_to_channels
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        events_to_channels(torch.zeros(3), torch.zeros(3), torch.ones(3), (4, 4))


def test_unsupported_shapes_fail_loudly():
    from models.BMCNet import BMCNet
    BMCNet(2, 16, 1)           # x2 SR (config/train_nfs.yml: SCALE 2/4/8): 4 sub-pixel channels, padded to the 16-channel granule
    with pytest.raises(NotImplementedError):
        BMCNet(3, 16, 1)       # odd scales: scale^2 is not a multiple of 4
    with pytest.raises(NotImplementedError):
        BMCNet(4, 8, 1)        # n_c = 8 is not a multiple of 16


def test_stacked_weight_cache_follows_parameter_versions():
    """ops.stacked: the stacked per-group weights (v1 / v2) are rebuilt exactly when one of the parameters changed (version
    counter) or is another object (ids can be recycled: weak references), never otherwise."""
    from bmc_hip import ops
    a, b = torch.nn.Parameter(torch.randn(4, 4)), torch.nn.Parameter(torch.randn(4, 4))
    calls = []

    def build():
        calls.append(1)
        return torch.stack([a.detach(), b.detach()])
    s0 = ops.stacked((a, b), build)
    assert ops.stacked((a, b), build) is s0 and len(calls) == 1
    with torch.no_grad():
        a.add_(1.0)                                  # what optimizer.step() does: same object, new version
    s1 = ops.stacked((a, b), build)
    assert s1 is not s0 and len(calls) == 2 and torch.equal(s1[0], a.detach())
    c = torch.nn.Parameter(torch.randn(4, 4))
    s2 = ops.stacked((c, b), lambda: torch.stack([c.detach(), b.detach()]))
    assert s2 is not s1 and torch.equal(s2[0], c.detach())
    assert ops.stacked((a, b), build) is s1 and len(calls) == 2


def test_split_wgrad_plan_of_multi_source_convolutions():
    """ops.split_wgrad (host logic, no launch): dense 128-channel sources without a batch map go to the Winograd weight-gradient
    kernel with their own column offset, everything else into one sub-spec over the SAME weight tensor; single-source and
    all-narrow convolutions are not split; the plan is cached per view set."""
    from bmc_hip import ops
    sp = ops.ConvSpec([list(range(0, 128)), list(range(128, 256)), list(range(256, 272)), list(range(272, 288))])
    plain = [(0, 128, 0, None, 0), (0, 128, 0, None, 4), (0, 16, 0, None, 0), (0, 16, 0, None, 4)]
    big, rest, sub = ops.split_wgrad(sp, plain)
    assert big == [(0, 0), (1, 128)] and rest == [2, 3]
    assert sub.cin == sp.cin and sub.kmap_host == list(range(256, 288)) and not sub.covers_all
    assert ops.split_wgrad(sp, plain) is ops.split_wgrad(sp, plain)
    big, rest, sub = ops.split_wgrad(sp, [(0, 128, 1, 8, 0)] + plain[1:])          # source 0 read through a batch rotation
    assert big == [(1, 128)] and rest == [0, 2, 3] and sub.kmap_host[:128] == list(range(0, 128))
    # padded narrow sources (conv_fpst: 6 real channels in a 16-channel window) keep their -1 entries in the sub-spec
    sp2 = ops.ConvSpec([list(range(0, 6)) + [-1] * 10, list(range(6, 134)), list(range(134, 150))])
    big, rest, sub = ops.split_wgrad(sp2, [(0, 16, 0, None, 0), (0, 128, 0, None, 0), (0, 16, 0, None, 0)])
    assert big == [(1, 6)] and rest == [0, 2] and sub.kmap_host[:8] == [0, 1, 2, 3, 4, 5, -1, -1] and sub.cin == 150
    assert ops.split_wgrad(ops.ConvSpec.dense(128), [(0, 128, 0, None, 0)]) is None
    assert ops.split_wgrad(ops.ConvSpec.dense(16, 32), [(0, 16, 0, None, 0), (0, 32, 0, None, 0)]) is None
