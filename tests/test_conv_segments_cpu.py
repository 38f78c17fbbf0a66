"""Operand descriptors on the host (no GPU): where ops._src puts every launch image, for plain, shifted / modular and
batch-segmented views (ops.View(t, t2=, seg=)), checked against the tensors' own addresses; and what View / _src refuse."""
import ctypes as C

import pytest
import torch

from bmc_hip import lib, ops
from bmc_hip.ops import View, _src

H, W, CT = 5, 7, 32


def image_base(s, b):
    """Byte address of launch image b of an operand: include/bmc_hip.h (bmc_src_t, bmc_conv_args_t::seg_b) in one line."""
    bs = (b + s.batch_shift) % s.batch_mod
    return s.ptr + 4 * (bs * s.batch_stride + (s.seg_delta if s.seg_b and b >= s.seg_b else 0))


def at(t, b, c0=0):
    return t[b].data_ptr() + 4 * c0


def test_plain_and_windowed_views():
    t = torch.zeros(6, H, W, CT)
    s = _src(t, 0, CT, 0, None, 0, 6)
    assert (s.pix_stride, s.nch, s.batch_stride, s.seg_b, s.seg_delta) == (CT, CT, H * W * CT, 0, 0)
    assert [image_base(s, b) for b in range(6)] == [at(t, b) for b in range(6)]
    s = View(t, c0=16, nch=16, b0=2).src(3)                  # channel window of batches 2..4
    assert s.nch == 16 and [image_base(s, b) for b in range(3)] == [at(t, 2 + b, 16) for b in range(3)]


def test_shifted_and_modular_views():
    t = torch.zeros(4, H, W, CT)
    s = View(t, shift=2, mod=4).src(4)                       # the swapped twin: b -> (b + 2) % 4
    assert [image_base(s, b) for b in range(4)] == [at(t, (b + 2) % 4) for b in range(4)]
    s = View(t, mod=2).src(4)                                # a shared operand: b -> b % 2
    assert [image_base(s, b) for b in range(4)] == [at(t, b % 2) for b in range(4)]
    s = View(t, shift=1).src(3)                              # no modulus given: none applies
    assert [image_base(s, b) for b in range(3)] == [at(t, b + 1) for b in range(3)]


@pytest.mark.parametrize("second_below", [False, True])
@pytest.mark.parametrize("seg,n2", [(3, 3), (2, 5), (5, 1)])
def test_segmented_views(second_below, seg, n2):
    pool = torch.zeros(seg + n2 + 3, H, W, CT)
    t, t2 = (pool[n2 + 3:], pool[:n2]) if second_below else (pool[:seg], pool[seg + 3:])
    B = seg + n2
    for c0, nch in ((0, CT), (16, 16)):
        s = View(t, c0=c0, nch=nch, t2=t2, seg=seg).src(B)
        assert s.seg_b == seg and (s.seg_delta < 0) == second_below and s.batch_shift == 0 and s.batch_mod >= B
        assert [image_base(s, b) for b in range(B)] == [at(t, b, c0) for b in range(seg)] + [at(t2, b, c0) for b in range(n2)]
    # a first tensor with more images than the split point: the launch reads its first `seg` ones only
    if not second_below:
        t = pool[:seg + 1]
        s = _src(t, 0, CT, 0, None, 0, B, t2, seg)
        assert [image_base(s, b) for b in range(B)] == [at(t, b) for b in range(seg)] + [at(t2, b) for b in range(n2)]
    # two halves of one buffer: a segment with delta 0 is the plain operand
    s = _src(pool[:seg], 0, CT, 0, None, 0, B, pool[seg:seg + n2], seg)
    assert s.seg_delta == 0 and [image_base(s, b) for b in range(B)] == [at(pool, b) for b in range(B)]


def test_segment_validation():
    t, t2 = torch.zeros(3, H, W, CT), torch.zeros(3, H, W, CT)
    with pytest.raises(ValueError, match="both"):
        View(t, t2=t2)
    with pytest.raises(ValueError, match="both"):
        View(t, seg=2)
    for kw in ({"shift": 1}, {"mod": 3}, {"b0": 1}):
        with pytest.raises(ValueError, match="shift / mod / b0"):
            View(t, t2=t2, seg=3, **kw)
        with pytest.raises(ValueError, match="shift / mod / b0"):
            _src(t, 0, CT, kw.get("shift", 0), kw.get("mod"), kw.get("b0", 0), 6, t2, 3)
    for other in (torch.zeros(3, H, W + 1, CT), torch.zeros(3, H, W, 2 * CT), torch.zeros(3, H, W, CT, dtype=torch.float64)):
        with pytest.raises(ValueError, match="agree"):
            View(t, t2=other, seg=3)
    for seg in (0, 4):                                       # outside the first tensor
        with pytest.raises(ValueError, match="split point"):
            View(t, t2=t2, seg=seg)
    for seg, B in ((3, 3), (3, 7), (0, 3)):                  # seg = B, more images than the second tensor has, seg = 0
        with pytest.raises(ValueError, match="split point"):
            _src(t, 0, CT, 0, None, 0, B, t2, seg)
    with pytest.raises(ValueError, match="contiguous"):
        _src(t, 0, CT, 0, None, 0, 6, torch.zeros(3, H, CT, W).permute(0, 1, 3, 2), 3)
    with pytest.raises(ValueError, match="no single-tensor description"):
        View(t, t2=t2, seg=3).meta()
    s = _src(t, 0, CT, 0, None, 0, 6, t2, 3)
    for fn in (lambda: ops._batch_window(s, 0, 3), lambda: ops.pgemm_raw(s, [s], 6, H, W, 9, 6, CT, CT, None)):
        with pytest.raises(ValueError, match="convolution launches only"):
            fn()


def test_conv_args_carry_the_segment():
    """The C ABI carries the segment at launch level: bmc_conv_args_t ends in seg_b and one delta per operand."""
    names = [f[0] for f in lib.ConvArgs._fields_]
    assert names[-4:] == ["seg_b", "src_seg_delta", "residual_seg_delta", "mask_seg_delta"]
    assert C.sizeof(lib.ConvArgs().src_seg_delta) == 8 * lib.MAX_SRC and C.sizeof(lib.Src) == 32


def test_pair_threshold(monkeypatch):
    """ops.pair_res: the two residual blocks share launches from PAIR_RES_MIN_TILES F(4x4) workgroup tiles per block (169 per
    180x240 image) -- the benchmark's 8 images do, a batch-1 window's 2 do not -- and never with the switch off."""
    monkeypatch.setattr(ops, "PAIR_RES", True)
    monkeypatch.setattr(ops, "PAIR_RES_MIN_TILES", 1024)
    assert [ops.pair_res(b, 180, 240) for b in (2, 4, 6, 7, 8)] == [False, False, False, True, True]
    assert not ops.pair_res(4, 36, 52) and not ops._pair_route(2, 180, 240, 128, 9)
    monkeypatch.setattr(ops, "PAIR_RES", False)
    assert not ops.pair_res(8, 180, 240)
