#!/usr/bin/env python3
"""Time of the background-activity noise filter (bmc_hip.encodings.event_noise_mask, ONE call of bmc_event_denoise) against the
torch composition it replaces on the same columns: tests/event_denoise_ref.py::mask_sorted, a stable sort of the composite key
pixel * n + index and eight searchsorted passes.  Shapes: 180x240 with 10^6 events and 720x1280 with 10^7 (the drifting-bar
stream of the tests, 30 % noise, one second long).

Every shape is measured in --procs fresh processes, one after another; each warms both forms up (--warmup calls), checks that
they give the same mask, then times --reps calls of each, alternating, with device events around every call, and reports its
median.  The parent prints, per shape, the median over the processes, their minimum and maximum, the ratio, the peak bytes of
temporaries each form allocates beyond its inputs (torch.cuda.max_memory_allocated around one call; the kernel's are its outputs:
keep and the band counts), and the device's clock as torch reports it before and after.

python tools/time_denoise.py [--shapes 180x240:1000000:2e-4,720x1280:10000000:1e-4] [--support 1] [--procs 3] [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bmcnet-esr_amd"), os.path.join(ROOT, "tests")]


def clock():
    """The device's current shader clock in MHz, or None where torch cannot read it."""
    import torch
    try:
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def child(H, W, n, dt, support, reps, warmup):
    import torch
    import event_denoise_ref as R
    from bmc_hip.encodings import event_noise_mask
    dev = torch.device("cuda:0")
    xs, ys, ts, _ = (torch.from_numpy(c).to(dev) for c in R.stream(H, W, n, 0.3, seed=H * W))
    forms = {"kernel": lambda: event_noise_mask(xs, ys, ts, (H, W), dt, support),
             "composition": lambda: R.mask_sorted(xs, ys, ts, H, W, dt, support)}
    clock0 = clock()
    for _ in range(warmup):
        out = {k: f() for k, f in forms.items()}
    torch.cuda.synchronize()
    assert torch.equal(out["kernel"], out["composition"]), "the two forms disagree"
    kept = int(out["kernel"].sum())
    del out
    peak = {}
    for k, f in forms.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        f()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():                           # alternating
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            z.record()
            z.synchronize()
            times[k].append(a.elapsed_time(z))
    print(json.dumps(dict(kept_share=kept / n, ms={k: statistics.median(v) for k, v in times.items()}, peak_bytes=peak,
                          clock_mhz=[clock0, clock()])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="180x240:1000000:2e-4,720x1280:10000000:1e-4", help="HxW:events:dt, comma-separated")
    ap.add_argument("--support", type=int, default=1)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        size, n, dt = a.child.split(":")
        H, W = (int(v) for v in size.split("x"))
        return child(H, W, int(n), float(dt), a.support, a.reps, a.warmup)
    for shape in a.shapes.split(","):
        runs = []
        for _ in range(a.procs):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--support", str(a.support), "--reps",
                                str(a.reps), "--warmup", str(a.warmup)], stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                raise SystemExit("the measuring process for %s failed (exit status %d)" % (shape, p.returncode))
            runs.append(json.loads(p.stdout.splitlines()[-1]))
        size, n, dt = shape.split(":")
        row = dict(size=size, events=int(n), dt=float(dt), support=a.support, processes=a.procs, reps=a.reps,
                   kept_share=round(runs[0]["kept_share"], 4), clock_mhz=[r["clock_mhz"] for r in runs])
        for k in ("kernel", "composition"):
            ms = [r["ms"][k] for r in runs]
            row[k + "_ms"] = round(statistics.median(ms), 4)
            row[k + "_ms_min_max"] = [round(min(ms), 4), round(max(ms), 4)]
            row[k + "_temporary_bytes"] = runs[0]["peak_bytes"][k]
        row["composition_over_kernel"] = round(row["composition_ms"] / row["kernel_ms"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
