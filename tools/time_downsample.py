#!/usr/bin/env python3
"""Time of the integrate-and-fire event downsampler (bmc_hip.encodings.downsample_events, include/bmc_hip_downsample.h): the
whole call (trim=False: nothing waits), the grouping sort alone (torch.sort(stable=True) of the int32 keys) and the library's own
launches alone (keys, walk, gather), on the drifting-bar stream of the tests (30 % noise, one second long).  Shapes: 10^6 events
at 720x960 -> 180x240 and 10^7 at 720x1280 -> 180x320, scale 4, threshold 16.

Every shape is measured in --procs fresh processes, one after another; each warms up (--warmup calls), then times --reps calls of
each piece, alternating, with device events around every call, and reports its median.  The parent prints, per shape, the median
over the processes, their minimum and maximum, the share of the whole call the sort takes, the bytes of the temporaries (keys,
their sorted copy, the permutation, fire, the chunk totals -- and the peak torch allocates around one call, the sort's own
workspace included), the LR events made, the longest and the mean segment the walk meets, and the device's clock as torch reports
it before and after.  For scale, the first process of a shape also runs the restatement's pixel-grouped numpy form
(tests/event_downsample_ref.py::downsample_grouped) on the host, once, and checks that the GPU gave the same bytes.

python tools/time_downsample.py [--shapes 720x960:1000000,720x1280:10000000] [--scale 4] [--threshold 16] [--procs 3] [--reps 10]
                                [--warmup 3] [--no-host]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bmcnet-esr_amd"), os.path.join(ROOT, "tests")]


def clock():
    """The device's current shader clock in MHz, or None where torch cannot read it."""
    import torch
    try:
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def child(H, W, n, s, T, reps, warmup, host):
    import numpy as np
    import torch
    import event_denoise_ref as N
    import event_downsample_ref as R
    from bmc_hip import downsample_lib as D, lib, ops
    from bmc_hip.encodings import downsample_events
    dev = torch.device("cuda:0")
    cols = N.stream(H, W, n, 0.3, seed=H * W)
    xs, ys, ts, ps = (torch.from_numpy(c).to(dev) for c in cols)
    h, w = R.lr_size(H, W, s)
    cap = D.capacity(n, T)
    keys, fire = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int8, device=dev)
    out = [torch.empty(cap, dtype=d, device=dev) for d in (torch.int16, torch.int16, torch.float64, torch.float64)]
    count = torch.empty(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(D.scratch_bytes(n) // 8, dtype=torch.int64, device=dev)
    st = ops._stream()
    run_keys = lambda: lib.call(D._keys, "keys", xs.data_ptr(), ys.data_ptr(), ps.data_ptr(), n, H, W, s, keys.data_ptr(),
                                fire.data_ptr(), st)
    run_keys()
    skeys, perm = torch.sort(keys, stable=True)
    run_walk = lambda: lib.call(D._walk, "walk", skeys.data_ptr(), perm.data_ptr(), ps.data_ptr(), n, H, W, s, T, fire.data_ptr(), st)
    run_gather = lambda: lib.call(D._gather, "gather", xs.data_ptr(), ys.data_ptr(), ts.data_ptr(), fire.data_ptr(), n, s,
                                  *(t.data_ptr() for t in out), cap, count.data_ptr(), scratch.data_ptr(), st)
    forms = {"call": lambda: downsample_events(xs, ys, ts, ps, (H, W), s, T, trim=False), "sort": lambda: torch.sort(keys, stable=True),
             "keys": run_keys, "walk": run_walk, "gather": run_gather}
    clock0 = clock()
    for _ in range(warmup):
        for f in forms.values():                             # (keys, walk, gather in this order leave fire as one call does)
            got = f()
    torch.cuda.synchronize()
    whole = downsample_events(xs, ys, ts, ps, (H, W), s, T)
    made = whole[0].numel()
    assert int(count.item()) == made and all(torch.equal(a, b[:made]) for a, b in zip(whole[:4], out)), "the pieces disagree with the call"
    seg = torch.bincount(skeys[skeys < h * w].long(), minlength=h * w)
    host_ms = None
    if host:
        t0 = time.perf_counter()
        want = R.downsample_grouped(*cols, H, W, s, T)
        host_ms = 1e3 * (time.perf_counter() - t0)
        assert R.same(want[:4], tuple(t.cpu().numpy() for t in whole[:4])), "the GPU and the host form disagree"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = forms["call"]()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del got
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():                           # alternating
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            z.record()
            z.synchronize()
            times[k].append(a.elapsed_time(z))
    print(json.dumps(dict(lr_events=made, ms={k: statistics.median(v) for k, v in times.items()}, host_ms=host_ms, peak_bytes=peak,
                          temporary_bytes=dict(keys=4 * n, sorted_keys=4 * n, permutation=8 * n, fire=n, totals=D.scratch_bytes(n)),
                          output_bytes=20 * cap + 8, longest_segment=int(seg.max()), mean_segment=float(seg.float().mean()),
                          clock_mhz=[clock0, clock()])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="720x960:1000000,720x1280:10000000", help="HxW:events of the HR stream, comma-separated")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--threshold", type=int, default=16)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="leave the host form (a Python loop over the events) out")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--host", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        size, n = a.child.split(":")
        H, W = (int(v) for v in size.split("x"))
        return child(H, W, int(n), a.scale, a.threshold, a.reps, a.warmup, a.host)
    for shape in a.shapes.split(","):
        runs = []
        for k in range(a.procs):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--scale", str(a.scale), "--threshold",
                   str(a.threshold), "--reps", str(a.reps), "--warmup", str(a.warmup)] + (["--host"] if k == 0 and not a.no_host else [])
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                raise SystemExit("the measuring process for %s failed (exit status %d)" % (shape, p.returncode))
            runs.append(json.loads(p.stdout.splitlines()[-1]))
        size, n = shape.split(":")
        row = dict(size=size, events=int(n), scale=a.scale, threshold=a.threshold, processes=a.procs, reps=a.reps,
                   lr_events=runs[0]["lr_events"], longest_segment=runs[0]["longest_segment"],
                   mean_segment=round(runs[0]["mean_segment"], 2), clock_mhz=[r["clock_mhz"] for r in runs])
        for k in ("call", "sort", "keys", "walk", "gather"):
            ms = [r["ms"][k] for r in runs]
            row[k + "_ms"] = round(statistics.median(ms), 4)
            row[k + "_ms_min_max"] = [round(min(ms), 4), round(max(ms), 4)]
        row["library_ms"] = round(row["keys_ms"] + row["walk_ms"] + row["gather_ms"], 4)
        row["sort_share"] = round(row["sort_ms"] / row["call_ms"], 3)
        row["host_grouped_numpy_ms"] = None if runs[0]["host_ms"] is None else round(runs[0]["host_ms"], 1)
        row["temporary_bytes"] = runs[0]["temporary_bytes"]
        row["output_bytes"] = runs[0]["output_bytes"]
        row["peak_bytes"] = runs[0]["peak_bytes"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
