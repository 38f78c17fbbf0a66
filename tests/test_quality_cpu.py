"""PSNR / SSIM of multi-stream inference, the parts that need no GPU: tests/quality_ref.py (the float64 oracle, a direct 49-term
window) against scikit-image's own formulation through scipy.ndimage.uniform_filter, which also gives the FLOOR the GPU bars
are built on; slots.quality_values on hand-made raw records; the refusals of Quality.check; the slot table's new trailing
section; the companion header against the library's ABI text and the binding."""
import math
import os

import numpy as np
import pytest

import quality_ref as Q


def _tiles():
    from bmc_hip import quality_lib
    return quality_lib.const("BMC_QUALITY_TILE_H"), quality_lib.const("BMC_QUALITY_TILE_W")


# ------------------------------------------------------------------ the oracle is scikit-image's definition
def _spread(a, g, rng):
    """The largest |mean SSIM (oracle) - mean SSIM (uniform_filter)| over the channels with a data range."""
    worst = 0.0
    for c, R in enumerate(Q.data_range(g, rng)):
        if R != 0:
            m1, m2 = Q.ssim_map(a[c], g[c], R), Q.ssim_map_uniform_filter(a[c], g[c], R)
            assert m1.shape == m2.shape == (a.shape[1] - 6, a.shape[2] - 6)
            assert np.abs(m1 - m2).max() <= 1e-12           # the maps themselves: rounding only
            worst = max(worst, abs(m1.mean() - m2.mean()))
    return worst


def test_oracle_equals_the_uniform_filter_formulation_and_floor_is_what_it_measures():
    measured = 0.0
    for h, w in Q.shapes(*_tiles()) + [(48, 80), (40, 72)]:     # the shapes of tests/test_gpu_quality.py, with its contents
        for lam in (3.0, 0.1):
            a, g = Q.make_images(h, w, seed=h * 1000 + w, lam=lam)
            for n in range(3):
                for rng in ("gt", 4.0):
                    measured = max(measured, _spread(a[n], g[n], rng))
    for h, w in ((7, 7), (8, 13), (40, 72), (48, 80)):           # integer counts up to 191, unrelated and near-equal images
        r = np.random.default_rng(h * w)
        g = r.integers(0, 192, (2, h, w)).astype(np.float32)
        for a in (r.integers(0, 192, g.shape).astype(np.float32), np.clip(g + r.integers(-3, 4, g.shape), 0, 191).astype(np.float32)):
            measured = max(measured, _spread(a, g, "gt"))
    print("spread between the two float64 formulations: %.3g (FLOOR %.3g, SSIM bar %.3g)" % (measured, Q.FLOOR, Q.SSIM_BAR))
    assert Q.FLOOR / 4 <= measured <= Q.FLOOR
    assert Q.SSIM_BAR == max(1000 * Q.FLOOR, 1e-13) <= 1e-10


def test_oracle_special_values():
    a, g = Q.make_images(9, 11, seed=5)
    psnr, ssim = Q.quality(a, g)
    assert np.isfinite(psnr[0]) and 0 < ssim[0] < 1
    assert psnr[1] == np.inf and ssim[1] == 1.0              # a == g bit for bit
    assert psnr[2] == -np.inf and np.isnan(ssim[2])          # channel 1 of g empty: R_1 = 0 with an error
    psnr4, ssim4 = Q.quality(a, g, 4.0)
    assert np.isfinite(psnr4).tolist() == [True, False, True] and np.isfinite(ssim4).all() and ssim4[1] == 1.0
    R = Q.data_range(g[0])
    assert R[0] == g[0, 0].max() - g[0].min() and R[1] == g[0, 1].max() - g[0].min()      # the minimum over both channels


# ------------------------------------------------------------------ the host's finishing
def test_quality_values_on_hand_made_records():
    from bmc_hip import slots
    h, w = 9, 12
    n, npos = h * w, (h - 6) * (w - 6)
    raw = np.array([
        [[2.0 * n, 5.0, 1.0, 0.5 * npos], [0.5 * n, 3.0, 1.0, 0.25 * npos]],       # finite
        [[0.0, 5.0, 0.0, 1.0 * npos], [0.0, 2.0, 0.0, 1.0 * npos]],                # exact
        [[1.0 * n, 4.0, 0.0, 0.5 * npos], [3.0 * n, 0.0, 0.0, np.nan]],            # R_1 = 0 with an error
        [[1.0 * n, 4.0, 0.0, 0.5 * npos], [0.0, 0.0, 0.0, np.nan]],                # R_1 = 0 without: 0 / 0
    ])
    psnr, ssim = slots.quality_values(raw, "gt", (h, w))
    assert psnr.dtype == ssim.dtype == np.float64 and psnr.shape == ssim.shape == (4,)
    assert psnr[0] == (10 * np.log10(16.0 / 2.0) + 10 * np.log10(4.0 / 0.5)) / 2 and ssim[0] == 0.375
    assert psnr[1] == np.inf and ssim[1] == 1.0
    assert psnr[2] == -np.inf and np.isnan(ssim[2])
    assert np.isnan(psnr[3]) and np.isnan(ssim[3])
    psnr, ssim = slots.quality_values(raw[:3], 2.0, (h, w))                          # a constant range: gt_max / gt_min are not read
    assert psnr[0] == (10 * np.log10(4.0 / 2.0) + 10 * np.log10(4.0 / 0.5)) / 2 and psnr[1] == np.inf
    assert psnr[2] == (10 * np.log10(4.0 / 1.0) + 10 * np.log10(4.0 / 3.0)) / 2
    want = Q.finish(raw, "gt", (h, w))
    got = slots.quality_values(raw.reshape(2, 2, 2, 4), "gt", (h, w))                # leading axes are kept
    assert got[0].shape == (2, 2) and np.array_equal(got[0].ravel(), want[0], equal_nan=True)
    assert np.array_equal(got[1].ravel(), want[1], equal_nan=True)
    import torch
    assert np.array_equal(slots.quality_values(torch.tensor(raw), "gt", (h, w))[0], want[0], equal_nan=True)
    for bad in (0.0, -1.0, math.inf, math.nan, "GT", None, True):
        with pytest.raises(ValueError, match="data_range"):
            slots.quality_values(raw, bad, (h, w))
    with pytest.raises(ValueError, match="at least 7 x 7"):
        slots.quality_values(raw, "gt", (6, 12))
    with pytest.raises(ValueError, match="raw records"):
        slots.quality_values(raw[..., :3], "gt", (h, w))
    assert slots.quality_tiles(7, 7) == 1
    TH, TW = _tiles()
    assert slots.quality_tiles(TH + 6, TW + 6) == 1 and slots.quality_tiles(TH + 7, TW + 7) == 4
    assert slots.quality_tiles(2 * TH + 9, 3 * TW + 11) == 12


# ------------------------------------------------------------------ the option's refusals
def test_quality_check_refusals():
    import torch
    from infer import MultiStreamSR
    from infer_parts import Quality
    who = "MultiStreamSR: "
    assert Quality.check(who, None) is None and Quality.check(who, True) == "gt"
    assert Quality.check(who, {"data_range": "gt"}) == "gt" and Quality.check(who, {"data_range": 4}) == 4.0
    assert type(Quality.check(who, {"data_range": np.float32(2.5)})) is float
    for bad, match in ((False, "None, True or a dict"), (1, "None, True or a dict"), ("gt", "None, True or a dict"),
                       (4.0, "None, True or a dict"), ({}, "lacks the key 'data_range'"),
                       ({"data_range": "gt", "win": 7}, "unknown key 'win'"), ({"range": 1.0}, "unknown key 'range'"),
                       ({"data_range": 0}, "finite positive"), ({"data_range": -2.0}, "finite positive"),
                       ({"data_range": math.inf}, "finite positive"), ({"data_range": math.nan}, "finite positive"),
                       ({"data_range": True}, "finite positive"), ({"data_range": "max"}, "finite positive"),
                       ({"data_range": None}, "finite positive")):
        with pytest.raises(ValueError, match=match):
            Quality.check(who, bad)
    m = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="MultiStreamSR: quality"):
        MultiStreamSR(m, 2, quality="yes")
    off, on = MultiStreamSR(m, 2), MultiStreamSR(m, 2, quality={"data_range": 3.0})
    assert off.quality is None and not any(type(p) is Quality for p in off.parts)
    kinds = [type(p).__name__ for p in on.parts]
    assert on.quality == 3.0 and kinds.index("Quality") == kinds.index("Metrics") + 1
    with pytest.raises(ValueError, match="at least 7 x 7"):
        Quality.check_size("open", 6, 40)
    Quality.check_size("open", 7, 7)


# ------------------------------------------------------------------ the slot table
def test_table_layout_gains_only_a_trailing_section():
    from bmc_hip import slots
    for S in (1, 5):
        for kw in ({}, dict(events=True), dict(events=True, hot=True, emit=True, timed=True, clock=True, render=5, voxel=True)):
            base = slots.table_layout(S, **kw)
            assert slots.table_layout(S, quality=False, **kw) == base
            sections, nbytes = slots.table_layout(S, quality=True, **kw)
            assert sections[:-1] == base[0] and sections[-1] == ("quality", slots.SLOT_QUALITY_DTYPE, base[1])
            assert nbytes == base[1] + 8 * S
    assert slots.table_layout(3) == ([("slot", slots.SLOT_DTYPE, 0)], 3 * slots.SLOT_DTYPE.itemsize)      # as it was
    positional = slots.table_layout(2, True, True, True, True, True, 2, True)
    assert [n for n, _, _ in positional[0]] == ["slot", "events", "emit", "clock", "hot", "render", "voxel"]
    with pytest.raises(ValueError, match="quality must be True or False"):
        slots.table_layout(2, quality=1)
    assert slots.QUALITY_LAUNCHES == 0 or isinstance(slots.QUALITY_LAUNCHES, int)
    assert set(slots.LAUNCHES) == {"stage", "commit", "metrics"}                    # the counter has a name of its own


# ------------------------------------------------------------------ the companion header and its binding
def test_companion_header_matches_its_abi_text_and_binding():
    """include/bmc_hip_quality.h by the routes tests/test_cabi_and_host.py takes for bmc_hip.h: the header's text (abi_ref's
    regular expressions and classes) and a C compile of it, against bmc_quality_abi() and what bmc_hip/quality_lib.py installs."""
    import ctypes as C
    import re
    import shutil
    import subprocess
    import tempfile
    import abi_ref
    from bmc_hip import lib, quality_lib, slots
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(abi_ref.INCLUDE, "bmc_hip_quality.h")).read(), flags=re.S)
    declared = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?[a-z][a-z ]*\*?)\s*\b(bmc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, re.M):
        params = [p.strip() for p in params.split(",")]
        declared[name] = [abi_ref.classify(ret)] + ([] if params == ["void"] else [abi_ref.classify(p) for p in params])
    assert sorted(declared) == sorted(quality_lib.FUNCTIONS) == ["bmc_quality_abi", "bmc_slot_quality"]
    assert not set(declared) & set(lib.FUNCTIONS) and not set(quality_lib.STRUCTS) & set(lib.STRUCTS)      # bmc_hip.h's tables do not grow
    ret, *params = declared["bmc_slot_quality"]
    fn = quality_lib._slot_quality
    assert [c.split(":")[0] for c in quality_lib.FUNCTIONS["bmc_slot_quality"]] == [ret] + params
    assert quality_lib.FUNCTIONS["bmc_slot_quality"][1:3] == ["p:bmc_slot_t", "p:bmc_slot_quality_t"]
    assert fn.restype is C.c_int and len(fn.argtypes) == len(params) == 12
    for kind, got in zip(params, fn.argtypes):
        assert got is {"p": C.c_void_p, "i4": C.c_int, "f8": C.c_double}[kind], kind
    assert [c.split(":")[0] for c in quality_lib.FUNCTIONS["bmc_quality_abi"]] == declared["bmc_quality_abi"] == ["p"]
    structs = re.findall(r"^\}\s*(bmc_[a-z0-9_]+_t)\s*;", text, re.M)
    assert structs == list(quality_lib.STRUCTS) == ["bmc_slot_quality_t"]
    names = re.findall(r"^#define[ \t]+(BMC_[A-Z0-9_]+)[ \t]+\S", text, re.M)
    assert sorted(names) == sorted(quality_lib.CONSTANTS) == ["BMC_QUALITY_STATS_WORDS", "BMC_QUALITY_TILE_H", "BMC_QUALITY_TILE_W",
                                                              "BMC_QUALITY_WIN", "BMC_QUALITY_WORDS"]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no host C compiler"
    body = ['printf("%s %%d\\n", (int)(%s));' % (n, n) for n in names]
    body += ['printf("sizeof %d\\n", (int)sizeof(bmc_slot_quality_t));', 'printf("dst %d\\n", (int)offsetof(bmc_slot_quality_t, dst));',
             'printf("dst_size %d\\n", (int)sizeof(((bmc_slot_quality_t*)0)->dst));']
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "bmc_hip_quality.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(body)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run([cc, "-I" + abi_ref.INCLUDE, os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    compiled = dict(zip(out[::2], map(int, out[1::2])))
    st = quality_lib.STRUCTS["bmc_slot_quality_t"]
    f = st.fields["dst"]
    assert (st.size, st.align, list(st.fields)) == (compiled.pop("sizeof"), 8, ["dst"])
    assert (f.offset, f.size, f.elem_size, f.code, f.shape) == (compiled.pop("dst"), compiled.pop("dst_size"), 8, "p", ())
    assert compiled == quality_lib.CONSTANTS and all(type(v) is int for v in quality_lib.CONSTANTS.values())
    assert compiled == {"BMC_QUALITY_WIN": 7, "BMC_QUALITY_WORDS": 4, "BMC_QUALITY_TILE_H": compiled["BMC_QUALITY_TILE_H"],
                        "BMC_QUALITY_TILE_W": compiled["BMC_QUALITY_TILE_W"], "BMC_QUALITY_STATS_WORDS": 8}
    dt = slots.SLOT_QUALITY_DTYPE
    assert dt == quality_lib.dtype("bmc_slot_quality_t") and dt.itemsize == 8 and dt.names == ("dst",) and dt.fields["dst"][0].str == "<u8"
    assert (slots.QUALITY_WIN, slots.QUALITY_WORDS, slots.QUALITY_STATS_WORDS) == (7, 4, 8)
    assert (slots.QUALITY_TILE_H, slots.QUALITY_TILE_W) == _tiles() and slots.QUALITY_KERNELS == 3
    assert lib.has_symbol("bmc_slot_quality") and lib.has_symbol("bmc_quality_abi")


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from bmc_hip import lib, quality_lib
    p = 4096                                                 # never dereferenced: every call below returns at its argument check
    ok = dict(table=p, quality=p, S=2, esr=p, bicubic=p, gh=9, gw=12, nparts=1, data_range=0.0, stats=p, tiles=p, s=None)

    def call(**kw):
        return quality_lib._slot_quality(*{**ok, **kw}.values())
    for kw in (dict(table=None), dict(quality=None), dict(esr=None), dict(stats=None), dict(tiles=None), dict(S=0), dict(S=257),
               dict(gh=6), dict(gw=6), dict(gh=1 << 15, gw=1 << 14), dict(nparts=0), dict(nparts=65), dict(data_range=-1.0),
               dict(data_range=math.inf), dict(data_range=math.nan), dict(stats=p + 4), dict(tiles=p + 4), dict(quality=p + 4),
               dict(esr=p + 2), dict(bicubic=p + 2)):
        assert call(**kw) == -1 and b"bmc_slot_quality" in lib.bmc_last_error(), kw
