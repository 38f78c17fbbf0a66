"""Times the four 3x3 weight-gradient launches of a C2 window (180x240, bs 4) that stay on the pixel-reduction GEMM: the narrow
"rest" sources of conv_fpst / conv_fps / conv_fs (shared part) and conv_o.  One line per shape: median, minimum and maximum of
REPS timings of ITERS back-to-back launches each (us per launch), and the wave map the launcher reports where it can.

  python tools/time_pgemm9_narrow.py [--root TREE]     TREE: another checkout with its own built library (A/B on one box)
"""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
sys.path.insert(0, os.path.join(args.root, "bmcnet-esr_amd"))
import torch  # noqa: E402
from bmc_hip import lib, ops  # noqa: E402
from bmc_hip.ops import _src, pgemm_raw  # noqa: E402

dev = torch.device("cuda:0")
H, W = 180, 240
# (name, images, M, physical widths of the X sources, bias partials)
SHAPES = [("conv_fpst rest", 8, 128, [16, 16], False), ("conv_fps rest", 8, 128, [16], False),
          ("conv_fs shared rest", 4, 128, [16, 16], False), ("conv_o", 4, 32, [128, 128], True)]
wave_map = getattr(lib, "pgemm_wave_map", None)
torch.manual_seed(0)
for name, B, M, widths, bias in SHAPES:
    a = torch.randn(B, H, W, M, device=dev)
    xs = [torch.randn(B, H, W, n, device=dev) for n in widths]
    N = sum(widths)
    fn = lambda: pgemm_raw(_src(a, 0, M, 0, None, 0, B), [_src(x, 0, n, 0, None, 0, B) for x, n in zip(xs, widths)], B, H, W, 9, B,
                           M, N, dev, want_bias=bias)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / args.iters * 1e3)
    ts.sort()
    print("%-20s B=%d M=%3d N=%3d KS=%s: median %7.1f us  min %7.1f  max %7.1f  (%.1f TFLOP/s real)" % (
        name, B, M, N, wave_map(9, M, N) if wave_map else "-", ts[len(ts) // 2], ts[0], ts[-1],
        2.0 * B * H * W * M * 9 * N / ts[len(ts) // 2] / 1e6), flush=True)
