#!/usr/bin/env python3
"""Multi-stream inference throughput (infer.MultiStreamSR): S recordings in the slots of one batched window, BMCNet(4,128,5),
eager and graph replay, next to StreamingSR at batch 1 in the same process.  Per configuration: the per-window latency
(median of the events around each window, the reference's `time` metric) and the aggregate windows/s (slot-windows over the
wall time of the timed windows, ended by a device synchronise; every slot busy in every timed window).

python tools/multistream_infer.py [--sizes 31x56,45x80,180x240] [--slots 1,8,32] [--windows 8] [--warmup 4] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bmcnet-esr_amd")]
import torch

from infer import MultiStreamSR, StreamingSR
from models.BMCNet import BMCNet

SEQN = 3


def streaming(m, frames, graph, warmup, windows):
    sr = StreamingSR(m, 128, 4, graph=graph)
    for i in range(warmup + windows):
        sr.step(frames[None, i:i + SEQN].transpose(1, 2))
    t = sr.times_ms[warmup:]
    return statistics.median(t), 1e3 * len(t) / sum(t)


def multistream(m, recs, S, graph, warmup, windows):
    ms = MultiStreamSR(m, S, n_c=128, scale=4, graph=graph, seqn=SEQN)
    hs = [ms.open(f, g) for f, g in recs[:S]]
    for _ in range(warmup):
        ms.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(windows):
        ms.step()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    lat = statistics.median(ms.results(hs[0])["time"][warmup:])
    return lat, S * windows / wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="31x56,45x80,180x240")
    ap.add_argument("--slots", default="1,8,32")
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = BMCNet(4, 128, 5).to(dev)
    rows = []
    L = a.warmup + a.windows + SEQN - 1
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        g = torch.Generator().manual_seed(H * W)
        slots = [int(s) for s in a.slots.split(",")]
        recs = [(torch.poisson(torch.full((L, 2, H, W), 0.284), generator=g).to(dev),
                 torch.poisson(torch.full((L, 2, 4 * H, 4 * W), 0.1), generator=g).to(dev)) for _ in range(max(slots))]
        for graph in (False, True):
            mode = "graph" if graph else "eager"
            lat, wps = streaming(m, recs[0][0], graph, a.warmup, a.windows)
            rows.append(dict(size=size, mode=mode, runner="StreamingSR", slots=1, ms_per_window=round(lat, 3),
                             windows_per_s=round(wps, 1)))
            print(json.dumps(rows[-1]), flush=True)
            for S in slots:
                lat, wps = multistream(m, recs, S, graph, a.warmup, a.windows)
                rows.append(dict(size=size, mode=mode, runner="MultiStreamSR", slots=S, ms_per_window=round(lat, 3),
                                 windows_per_s=round(wps, 1)))
                print(json.dumps(rows[-1]), flush=True)
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
