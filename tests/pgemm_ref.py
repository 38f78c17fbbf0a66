"""Plain restatement of the pixel-reduction GEMM of include/bmc_hip.h (bmc_pgemm; kernels in csrc/pgemm.hip, csrc/pgemm_bf.hip):

    C[g][tap][m][n] = sum_{b in group g} sum_{y,x} A[b,y,x,m] * cat(src)[b, y+dy, x+dx, n]        tap = 3 (dy + 1) + (dx + 1)

written with explicit tap shifts and zero padding (no convolution routine), torch on the CPU in float64, no tiling and no fixed
summation order.  Next to C it returns what the bars of tests/test_gpu_pgemm_kernels.py are made of: sum |a x| per element (the
`absolute` convention of tests/weight_path_ref.py), the number of in-image products per element, and the bias gradient
sum_{b,y,x} A[b,y,x,m] per group with its sum |a|.  tests/test_pgemm_ref_cpu.py ties it to F.conv2d's autograd and torch.bmm.

It also restates, from the entry point's dispatch (bmc_pgemm in csrc/pgemm.hip, bmc_pgemm_bf_launch in csrc/pgemm_bf.hip), which
kernel instantiation a launch takes (`kernel_name`), and holds the case table both test files use (`CASES`): the smallest shapes
that reach each branch of the kernels.  `defect=` plants one of five defects a tiled kernel could have (DEFECTS); the CPU test
checks that each of them breaks the GPU test's bars."""
import zlib
from collections import namedtuple

import torch

F64 = torch.float64
MAX_SRC = 6                     # BMC_MAX_SRC
PT_H, PT_W, PT = 4, 16, 64      # pixel tile: 3x3 launches 4 rows x 16 columns, 1x1 launches 64 flat pixels
U32 = 2.0 ** -24                # unit roundoff of fp32


def pad32(v):
    return (v + 31) // 32 * 32


class Operand:
    """One operand of a launch.  Either a channel window [c0, c0 + nch) of an NHWC tensor t [Bt][H][W][Ct] whose image
    (b + shift) % mod launch image b reads (mod None: no wrapping), or -- a table operand -- a list `images` of per-image tensors
    [H][W][Ct], one per launch image, read through the same channel window."""

    def __init__(self, t=None, c0=0, nch=None, shift=0, mod=None, images=None):
        assert (t is None) != (images is None)
        self.t, self.images, self.c0, self.shift, self.mod = t, images, c0, shift, mod
        ct = (t if t is not None else images[0]).shape[-1]
        self.nch = ct - c0 if nch is None else nch

    def image(self, b):
        if self.images is not None:
            img = self.images[b]
        else:
            bs = b + self.shift
            img = self.t[bs % self.mod if self.mod is not None else bs]
        return img[..., self.c0:self.c0 + self.nch].to(F64)


def tap_shift(taps, tap):
    return (tap // 3 - 1, tap % 3 - 1) if taps == 9 else (0, 0)


def shifted(X, dy, dx):
    """out[b,y,x,:] = X[b,y+dy,x+dx,:] where that pixel lies in the image, 0 elsewhere (zero padding)."""
    H, W = X.shape[1], X.shape[2]
    out = torch.zeros_like(X)
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[:, y0:y1, x0:x1] = X[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def in_image_products(taps, tap, bpg, H, W):
    dy, dx = tap_shift(taps, tap)
    return bpg * max(0, H - abs(dy)) * max(0, W - abs(dx))


DEFECTS = ("drop_pixel", "dup_pixel", "tap_shift", "col_off4", "wrong_group")
Result = namedtuple("Result", "C absC count db absdb")


def pgemm(a, srcs, B, H, W, taps, bpg, defect=None):
    """-> Result(C [G][taps][M][N], sum |a x| of the same shape, in-image products per element (same shape), db [G][M], sum |a|
    [G][M]), all float64.  defect: one of DEFECTS, planted into group 0 (tap_shift: the last tap; col_off4: the first 32 columns)."""
    assert taps in (1, 9) and B % bpg == 0 and 1 <= len(srcs) <= MAX_SRC and defect in (None,) + DEFECTS
    G, M, N = B // bpg, a.nch, sum(s.nch for s in srcs)
    C, absC = torch.zeros(G, taps, M, N, dtype=F64), torch.zeros(G, taps, M, N, dtype=F64)
    count = torch.zeros(G, taps, M, N, dtype=F64)
    db, absdb = torch.zeros(G, M, dtype=F64), torch.zeros(G, M, dtype=F64)
    for g in range(G):
        imgs = list(range(g * bpg, (g + 1) * bpg))
        if defect == "wrong_group" and g == 0:
            assert G >= 2
            imgs[0] = bpg                                           # the first image of group 1
        A = torch.stack([a.image(b) for b in imgs])                 # [bpg][H][W][M]
        X = torch.stack([torch.cat([s.image(b) for s in srcs], -1) for b in imgs])      # [bpg][H][W][N]
        assert A.shape == (bpg, H, W, M) and X.shape == (bpg, H, W, N)
        if defect in ("drop_pixel", "dup_pixel") and g == 0:
            A = A.clone()
            A[0, H // 2, W // 2] *= 0.0 if defect == "drop_pixel" else 2.0
        if defect == "col_off4" and g == 0:
            X = X.clone()
            X[..., :min(32, N)] = torch.roll(X, -4, -1)[..., :min(32, N)]
        for tap in range(taps):
            dy, dx = tap_shift(taps, tap)
            if defect == "tap_shift" and g == 0 and tap == taps - 1:
                dx += 1
            Xs = shifted(X, dy, dx)
            C[g, tap] = torch.einsum("byxm,byxn->mn", A, Xs)
            absC[g, tap] = torch.einsum("byxm,byxn->mn", A.abs(), Xs.abs())
            count[g, tap] = in_image_products(taps, tap, bpg, H, W)
        db[g], absdb[g] = A.sum((0, 1, 2)), A.abs().sum((0, 1, 2))
    return Result(C, absC, count, db, absdb)


# ------------------------------------------------------------------ the launcher's choice of kernel
def wave_map(taps, M, N):
    """bmc_pgemm_wave_map: k-step shares of an fp32 launch with all taps per workgroup."""
    if taps != 9:
        return 1
    if pad32(M) <= 32:
        return 4
    return 2 if pad32(N) <= 32 else 1


def kernel_name(math, taps, tap_groups, table, M, N):
    """The instantiation bmc_pgemm launches.  math: 0 fp32, 1 bf16, 3 bf16x6 (BMC_MATH_*); tap_groups: 0 / 1 / 3 as in the argument
    block; table: any operand is a BMC_SRC_TABLE one.  (math 1 with tap_groups 3 is a run-time branch of bf<9,1>.)"""
    assert math in (0, 1, 3) and taps in (1, 9) and tap_groups in (0, 1, 3)
    assert tap_groups != 3 or (taps == 9 and math != 3)
    tab = ",tab" if table else ""
    if math == 3:
        return ("bf9x3<tab>" if table else "bf9x3") if taps == 9 else "bf<1,3%s>" % tab
    if math == 1:
        return "bf<%d,1%s>" % (taps, tab)
    if taps == 1:
        return "dma<1,1%s>" % tab
    if tap_groups == 3:
        return "dma<9,3%s>" % tab
    ks = wave_map(9, M, N)
    return "dma<9,9%s%s>" % (tab, ",ks%d" % ks if ks > 1 else "")


DMA_KERNELS = ["dma<9,9>", "dma<9,9,tab>", "dma<9,3>", "dma<9,3,tab>", "dma<9,9,ks2>", "dma<9,9,tab,ks2>", "dma<9,9,ks4>",
               "dma<9,9,tab,ks4>", "dma<1,1>", "dma<1,1,tab>"]
BF_KERNELS = ["bf9x3", "bf9x3<tab>", "bf<1,3>", "bf<1,3,tab>", "bf<9,1>", "bf<9,1,tab>", "bf<1,1>", "bf<1,1,tab>"]
ALL_KERNELS = DMA_KERNELS + BF_KERNELS


# ------------------------------------------------------------------ the case table
Shape = namedtuple("Shape", "taps M widths B bpg H W bias shift mod")


def _s(taps, M, widths, B, bpg, H, W, bias, shift=0, mod=None):
    return Shape(taps, M, tuple(widths), B, bpg, H, W, bias, shift, mod)


SHAPES = {
    # 1x1 (tiles of 64 flat pixels)
    "a": _s(1, 128, [128], 1, 1, 5, 13, False),                 # 65 pixels: a full tile + a one-pixel tile
    "b": _s(1, 48, [16, 48], 2, 2, 7, 19, True),                # 3 tiles per image, Mpad = 64 (idle waves), bias with M < Mpad
    "c": _s(1, 160, [64, 192, 16], 2, 2, 8, 16, True),          # two row blocks; column block 1 = source 1 from its column 64 on
    "d": _s(1, 128, [128], 3, 1, 6, 11, False, shift=1, mod=3),  # Gram form, G = B; the source rotated over the batch
    "e": _s(1, 32, [32], 4, 2, 8, 8, False),                    # two groups of two images
    "r": _s(1, 128, [128], 1, 1, 16, 16, True),                 # 4 full tiles: the uniform-base fill into re-used buffers
    "n": _s(1, 32, [32], 2, 2, 1, 1, True),                     # one-pixel images
    "q1": _s(1, 64, [16] * 6, 2, 2, 5, 18, True),               # BMC_MAX_SRC sources: the whole source walk
    "o": _s(1, 132, [32], 2, 2, 5, 13, True),                   # bias over two row blocks with M < Mpad = 160
    # 3x3 (tiles of 4 rows x 16 columns)
    "g": _s(9, 128, [64], 1, 1, 13, 50, True),                  # 4 x 4 tiles, 4 of them interior (uniform-base fill)
    "h": _s(9, 48, [48, 32], 2, 2, 9, 21, True),                # two column blocks, the second 16 wide; 6 tiles per image
    "i1": _s(9, 64, [64], 2, 2, 1, 1, True),
    "i3": _s(9, 64, [64], 2, 2, 3, 5, True),
    "m": _s(9, 48, [48], 4, 2, 5, 18, True),                    # two groups of two images
    "q9": _s(9, 64, [16] * 6, 2, 2, 5, 18, True),               # BMC_MAX_SRC sources: the whole source walk
    "p": _s(9, 132, [32], 2, 2, 9, 21, True),                   # bias over two row blocks with M < Mpad = 160, on the KS = 2 map
}
WAVE_SHAPES = []                # (j): the k-step-share wave maps, KS = 2 and KS = 4
for _M, _w in ((128, [16]), (48, [32]), (32, [32]), (16, [128]), (32, [256])):
    for _H, _W in ((9, 21), (13, 50)):
        _name = "j%dx%d_%dx%d" % (_M, sum(_w), _H, _W)
        SHAPES[_name] = _s(9, _M, _w, 2, 2, _H, _W, True)
        WAVE_SHAPES.append(_name)

Case = namedtuple("Case", "shape nsplit math tab tap_groups data")     # tab: "" plain, "all" every operand a table, "a" only A


def case_id(c):
    return "%s-ns%d-m%d%s%s-%s" % (c.shape, c.nsplit, c.math, "-tab" + c.tab if c.tab else "", "-tg3" if c.tap_groups == 3 else "",
                                   c.data)


def _cases():
    out = []

    def add(shape, nsplit, math=0, tab="", tg=1, data="int"):
        c = Case(shape, nsplit, math, tab, tg, data)
        if c not in out:
            out.append(c)

    for data in ("int", "randn"):                       # fp32: integer operands (exact) and randn (the first-order bound)
        for ns in (1, 2, 3):
            add("a", ns, data=data)                     # (a) nsplit 3: the third split is empty
        add("b", 4, data=data)                          # (b) the tile walk steps across images
        add("b", 1, data=data)                          #     6 tiles in one split: both LDS buffers are filled a second time
        add("b", 1, tab="all", data=data)
        add("r", 1, data=data)                          #     the same through the uniform-base fill
        add("c", 2, data=data)                          # (c)
        add("d", 2, data=data)                          # (d)
        add("e", 1, data=data)                          # (e)
        add("n", 3, data=data)                          #     one-pixel images, one empty split
        add("o", 2, data=data)                          #     bias partials of a second, partly padded row block
        add("p", 3, data=data)
        add("q1", 2, data=data)                         #     six sources
        add("q9", 2, data=data)
        add("h", 7, tab="a", data=data)                 #     3x3 with A a table and the sources plain
        for tab in ("all", "a"):                        # (f)
            add("b", 4, tab=tab, data=data)
            add("c", 2, tab=tab, data=data)
        for ns in (1, 5, 16):
            add("g", ns, data=data)                     # (g)
        add("h", 7, data=data)                          # (h) nsplit above one image's 6 tiles
        add("g", 5, tab="all", data=data)               #     the all-taps 4 x 2 map with tables
        add("h", 7, tab="all", data=data)
        add("i1", 3, data=data)                         # (i) 2 tiles, 3 splits
        add("i3", 2, data=data)
        add("m", 3, data=data)                          #     two groups, 3x3
        for s in WAVE_SHAPES:                           # (j)
            add(s, 3, data=data)
            add(s, 3, tab="all", data=data)
        for tab in ("", "all"):                         # (k) one tap row per workgroup, fp32
            add("g", 5, tab=tab, tg=3, data=data)
            add("h", 7, tab=tab, tg=3, data=data)
        add("j128x16_9x21", 3, tg=3, data=data)         #     the 4 x 2 map on shapes that leave a column / three row blocks idle
        add("j32x32_9x21", 3, tg=3, data=data)
    for tab in ("", "all"):
        add("g", 5, math=1, tab=tab, tg=3)              # (k) one tap row per workgroup, bf16
        add("h", 7, math=1, tab=tab, tg=3)
        for math in (1, 3):                             # (l) integer operands on the bf16 kernels
            add("g", 5, math=math, tab=tab)
            add("h", 7, math=math, tab=tab)
            add("b", 4, math=math, tab=tab)
            add("c", 2, math=math, tab=tab)
            add("b", 1, math=math, tab=tab)             #     6 tiles in one split: the 1x1 kernels' two-tile register ring refills
            add("r", 1, math=math, tab=tab)             #     the same through the uniform-base loads
        add("o", 2, math=3, tab=tab)                    #     their bias partials with a second, partly padded row block
        add("p", 3, math=3, tab=tab)
        for math in (1, 3):
            add("n", 3, math=math, tab=tab)             #     a split without tiles on the bf16 kernels
            add("i1", 3, math=math, tab=tab)
            add("q1", 2, math=math, tab=tab)            #     six sources
            add("q9", 2, math=math, tab=tab)
        for s, ns in (("b", 4), ("b", 1), ("c", 2), ("g", 5), ("h", 7)):      # bf16x6 on randn: the rel-L2 bar
            add(s, ns, math=3, tab=tab, data="randn")
    return out


CASES = _cases()


def case_kernel(c):
    s = SHAPES[c.shape]
    return kernel_name(c.math, s.taps, c.tap_groups, bool(c.tab), s.M, sum(s.widths))


def tiles_per_image(s):
    return ((s.H + PT_H - 1) // PT_H) * ((s.W + PT_W - 1) // PT_W) if s.taps == 9 else (s.H * s.W + PT - 1) // PT


def operands(shape, data):
    """The logical operands of a shape: (a [B][H][W][M], [x_i [Bx][H][W][n_i]]), float32 holding integers in [-8, 8] ("int") or
    randn; the same values whatever the launch's nsplit, math mode or operand kind.  Bx = B, or the batch modulus of the shape."""
    s = SHAPES[shape]
    g = torch.Generator().manual_seed(zlib.crc32(("%s/%s" % (shape, data)).encode()))
    Bx = s.mod if s.mod is not None else s.B

    def draw(*dims):
        if data == "int":
            return torch.randint(-8, 9, dims, generator=g).float()
        return torch.randn(*dims, generator=g)

    return draw(s.B, s.H, s.W, s.M), [draw(Bx, s.H, s.W, n) for n in s.widths]


_REF = {}


def reference(shape, data):
    """pgemm() of a shape's logical operands, computed once per (shape, data) and shared; callers must not modify it."""
    key = (shape, data)
    if key not in _REF:
        s = SHAPES[shape]
        a, xs = operands(shape, data)
        _REF[key] = pgemm(Operand(a), [Operand(x, shift=s.shift, mod=s.mod) for x in xs], s.B, s.H, s.W, s.taps, s.bpg)
    return _REF[key]
