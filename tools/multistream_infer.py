#!/usr/bin/env python3
"""Multi-stream inference throughput (infer.MultiStreamSR): S recordings in the slots of one batched window, BMCNet(4,128,5),
eager and graph replay, next to StreamingSR at batch 1 in the same process.  Per configuration: the per-window latency
(median of the events around each window, the reference's `time` metric) and the aggregate windows/s (slot-windows over the
wall time of the timed windows, ended by a device synchronise; every slot busy in every timed window).
--events adds, per configuration, the same session on EVENT-BACKED recordings (open_events: synthetic raw columns, LR blocks of
2 048 events advancing by 1 024, ground-truth blocks of 32 768): its latency and windows/s, the encode launch alone
(bmc_slot_encode on the session's last table, events around 20 launches) with its share of the window, and the bytes one
recording keeps on the GPU either way.
--emit-events adds, per configuration, the frame-backed session with the event OUTPUT on (emit_events=True): its latency and
windows/s, the bmc_slot_emit call alone (both kernels, events around 20 calls on the session's last table and prediction),
the events of its last window, and the bytes the recording keeps resident with events against with dense predictions.
--no-gt adds, per configuration, the frame-backed session on recordings WITHOUT ground truth (open(frames)): no metrics launch.
--sensor-clock (implies --emit-events --event-times) opens the emitting session's recordings with synthetic monotone float64
stamps (microseconds around 1e9, one frame every 33 333 us): float64 times on the sensor's clock, bmc_slot_emit_clocked.
--hot-filter (implies --events) adds, per configuration, the event-backed session with the hot-pixel filter on
(hot_filter=dict(max_px=100, min_obvs=5, max_rate=0.8), the reference's defaults) and off, --runs alternating runs each in this
process (windows/s: the median, and every run), and the bmc_slot_hot_update call alone (events around 20 calls on the session's
last table).
--noise-filter DT[:K] (implies --events) adds, per configuration, the event-backed session on recordings with a known share of
uniform noise events (a drifting bar, one second long, 20 % noise) opened with noise_filter=dict(ts=, dt=DT, support=K) and without,
--runs alternating runs each: the share of the LR events the filter dropped next to the share that is noise, the mean esr_mse of
both, and ms per window and windows/s of both (the filter runs once per recording at open_events: nothing enters a window).
--from-hr [T] adds, per configuration, the event-backed session on HR-ONLY recordings (open_hr_events: the LR stream is made at the
door, on the GPU, by integrate-and-fire over 4 x 4 blocks with threshold T, default 16; include/bmc_hip_downsample.h) with PSNR /
SSIM on: ms per window, windows/s, the LR events synthesized per HR event, ms of open_hr_events per recording (the synthesis, its
one host sync and both index tables) and the means of esr_mse, esr_psnr and esr_ssim -- the table from recordings that have no LR half.
--render DIR [--render-kinds lr,bicubic,esr,gt] adds, per configuration, the frame-backed session with the event-count images on
(render=kinds): its latency and windows/s, one bmc_slot_render call alone per kind (both kernels, events around 20 calls on the
session's last table), and writes the images of the first such session as DIR/<recording>/event_img/<kind dir>/%09d.png with the
reference's directory names (lr_event_img, hr_bicubic_event_img, hr_esr_event_img, hr_gt_event_img).  A file holds the rendered
array itself, one pixel per element; the reference's files are the same array resampled by matplotlib at 300 dpi.
--voxel-bins B adds, per configuration, the frame-backed session with the per-window voxel grids on (voxel_bins=B) and off, --runs
alternating runs each in this process (windows/s: the median, and every run), the bmc_slot_voxel call alone (both kernels, events
around 20 calls on the session's last table and prediction) and, for the same predictions, the composition it replaces: the timed
event stream of every slot (counts_to_events(times="linear")) and events_to_voxel_torch on its columns, slot by slot.
--self-ensemble K [--plain-weights NPZ] adds, per configuration whose slot count K divides, the session with self_ensemble=K and the
one without, --runs alternating runs each, on structured synthetic recordings (drifting bars: the ground truth is the Poisson counts
of an HR rate field, an LR frame those of its 4 x 4 block means): RECORDING windows/s of both (with the option a recording takes K
slots) and the mean esr_mse of the recordings both ran.  --plain-weights: BMCNet_plain(4,128,5) with the parameters of the file.
--quality [RANGE] adds, per configuration, the frame-backed session with PSNR / SSIM on (quality=True, or dict(data_range=RANGE) with a
number) and off, --runs alternating runs each in this process (ms per window and windows/s: the median, and every run), the quality
part's launches alone (the resizes, the frame-1 copy and bmc_slot_quality's three kernels, events around 20 calls on the session's
last table and prediction) and the means of esr_psnr, esr_ssim, bicubic_psnr and bicubic_ssim over the recordings' finite windows.
--resident-windows N prints, per size, what an event-backed recording of N windows keeps resident with dense predictions and
with the event output (nothing is run: the buffers are allocated when a recording is opened).

python tools/multistream_infer.py [--sizes 31x56,45x80,180x240] [--slots 1,8,32] [--windows 8] [--warmup 4] [--events]
                                  [--hot-filter] [--noise-filter DT[:K]] [--from-hr [T]] [--runs 3]
                                  [--emit-events] [--event-times] [--sensor-clock] [--continuous] [--no-gt] [--resident-windows N] [--modes eager,graph] [--out FILE]
                                  [--render DIR] [--render-kinds lr,bicubic,esr,gt] [--voxel-bins B]
                                  [--self-ensemble K] [--plain-weights NPZ] [--quality [RANGE]]"""
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
from infer_parts import EventStream, HotFilter, Input, Pictures, Quality, VoxelGrids
from models.BMCNet import BMCNet

SEQN = 3


def streaming(m, frames, graph, warmup, windows):
    sr = StreamingSR(m, 128, 4, graph=graph)
    for i in range(warmup + windows):
        sr.step(frames[None, i:i + SEQN].transpose(1, 2))
    t = sr.times_ms[warmup:]
    return statistics.median(t), 1e3 * len(t) / sum(t)


def event_recording(L, H, W, seed):
    """Synthetic raw columns of L items on the CPU -> the arguments of open_events."""
    import numpy as np
    from bmc_hip.encodings import event_window_indices
    rng = np.random.default_rng(seed)
    n_lr = 1024 * L + 1
    n_gt = 16 * n_lr
    cols = []
    for n, h, w in ((n_lr, H, W), (n_gt, 4 * H, 4 * W)):
        cols.append((torch.from_numpy(rng.integers(0, w, n).astype(np.int16)), torch.from_numpy(rng.integers(0, h, n).astype(np.int16)),
                     torch.from_numpy(rng.choice([-1.0, 1.0], n))))
    lr_index, gt_index = event_window_indices(np.sort(rng.uniform(0, 1, n_lr)), np.sort(rng.uniform(0, 1, n_gt)), 2048, 1024, 4)
    return cols[0], cols[1], lr_index, gt_index, (H, W), (4 * H, 4 * W)


NOISE_SHARE = 0.2


def noisy_event_recording(L, H, W, seed):
    """event_recording with a structured LR stream on a clock: a bar two pixels wide crosses the sensor once in one second, and a
    known share NOISE_SHARE of the events is uniform noise instead -> the arguments of open_events, then the float64 timestamp
    column and the number of noise events."""
    import numpy as np
    from bmc_hip.encodings import event_window_indices
    rng = np.random.default_rng(seed)
    n_lr = 1024 * L + 1
    n_gt = 16 * n_lr
    ts = np.sort(rng.uniform(0, 1, n_lr))
    noise = rng.random(n_lr) < NOISE_SHARE
    bar = np.minimum(np.floor(ts * max(W - 1, 1)).astype(np.int64) + rng.integers(0, 2, n_lr), W - 1)
    lr = (torch.from_numpy(np.where(noise, rng.integers(0, W, n_lr), bar).astype(np.int16)),
          torch.from_numpy(rng.integers(0, H, n_lr).astype(np.int16)), torch.from_numpy(rng.choice([-1.0, 1.0], n_lr)))
    gt = (torch.from_numpy(rng.integers(0, 4 * W, n_gt).astype(np.int16)), torch.from_numpy(rng.integers(0, 4 * H, n_gt).astype(np.int16)),
          torch.from_numpy(rng.choice([-1.0, 1.0], n_gt)))
    lr_index, gt_index = event_window_indices(ts, np.sort(rng.uniform(0, 1, n_gt)), 2048, 1024, 4)
    return lr, gt, lr_index, gt_index, (H, W), (4 * H, 4 * W), torch.from_numpy(ts), int(noise.sum())


def noise_session(m, recs, S, graph, warmup, windows, noise_filter):
    """The event-backed session on noisy_event_recording()s with open_events(noise_filter=dict(ts=, dt=, support=)) (noise_filter =
    (dt, support)) or without (None) -> median ms per window of the first recording, windows / s, the mean esr_mse of the timed
    windows, the share of the LR events the filter dropped (None without it)."""
    dev = next(m.parameters()).device
    ms = MultiStreamSR(m, S, n_c=128, scale=4, graph=graph, seqn=SEQN)
    hs = []
    for r in recs[:S]:
        nf = None if noise_filter is None else dict(ts=r[6].to(dev), dt=noise_filter[0], support=noise_filter[1])
        hs.append(ms.open_events(tuple(t.to(dev) for t in r[0]), tuple(t.to(dev) for t in r[1]), *r[2:6], noise_filter=nf))
    for _ in range(warmup):
        ms.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(windows):
        ms.step()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    res = [ms.results(h) for h in hs]
    mse = statistics.mean(v for r in res for v in r["esr_mse"][warmup:])
    dropped = None if noise_filter is None else sum(r["noise_events"] for r in res) / sum(r[0][0].numel() for r in recs[:S])
    return statistics.median(res[0]["time"][warmup:]), S * windows / wall, mse, dropped


def hr_recording(L, H, W, seed):
    """An HR-only recording on the CPU that gives at least L LR items of 2 048 events advancing by 1 024: uniform positions on the
    4H x 4W sensor, one second long, the polarity of an event fixed by its LR pixel (a checkerboard), so that every LR pixel fires
    once per 16 of its events -> (xs, ys, ps), the float64 timestamp column, (4H, 4W)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    n = 16 * (1024 * L + 1) + 16 * H * W
    xs, ys = rng.integers(0, 4 * W, n), rng.integers(0, 4 * H, n)
    ps = np.where((xs // 4 + ys // 4) % 2 == 0, 1.0, -1.0)
    return ((torch.from_numpy(xs.astype(np.int16)), torch.from_numpy(ys.astype(np.int16)), torch.from_numpy(ps)),
            torch.from_numpy(np.sort(rng.uniform(0, 1, n))), (4 * H, 4 * W))


def hr_session(m, recs, S, graph, warmup, windows, threshold):
    """The event-backed session on hr_recording()s opened with open_hr_events, quality on -> median ms per window of the first
    recording, windows / s, LR events per HR event, median ms of open_hr_events, the means of esr_mse, esr_psnr, esr_ssim over the
    timed windows (finite values)."""
    import math
    dev = next(m.parameters()).device
    ms = MultiStreamSR(m, S, n_c=128, scale=4, graph=graph, seqn=SEQN, quality=True)
    hs, door = [], []
    for gt, gt_ts, gt_size in recs[:S]:
        gt, gt_ts = tuple(t.to(dev) for t in gt), gt_ts.to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hs.append(ms.open_hr_events(gt, gt_ts, gt_size, threshold=threshold, dataset_length=warmup + windows + SEQN - 1))
        torch.cuda.synchronize()
        door.append(1e3 * (time.perf_counter() - t0))
    for _ in range(warmup):
        ms.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(windows):
        ms.step()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    res = [ms.results(h) for h in hs]
    mean = lambda k: statistics.mean([v for r in res for v in r[k][warmup:] if math.isfinite(v)] or [float("nan")])
    made = sum(r["synthesized_events"] for r in res) / sum(r[0][0].numel() for r in recs[:S])
    return (statistics.median(res[0]["time"][warmup:]), S * windows / wall, made, statistics.median(door), mean("esr_mse"),
            mean("esr_psnr"), mean("esr_ssim"))


def alone(call, reps=20):
    """ms per call() on the launch stream: events around `reps` calls, after one untimed call."""
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call()
    a.record()
    for _ in range(reps):
        call()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) / reps


def part_alone(ms, part):
    """ms per call of the launches of the session's part `part` (a class of infer_parts: Input = bmc_slot_encode, HotFilter =
    bmc_slot_hot_update, EventStream = bmc_slot_emit / _timed / _clocked, VoxelGrids = bmc_slot_voxel) on the session's buffers, with
    the part's own argument lists.  The calls repeat the last window: they count its item again, append nothing, rewrite its grids."""
    return alone(lambda: ms.part(part).launch(ms, ms._bufs, ms._bufs["pred"]))


HOT_FILTER = dict(max_px=100, min_obvs=5, max_rate=0.8)


def voxel_composition(ms):
    """ms of the composition bmc_slot_voxel replaces, on the session's last predictions: their timed stream (counts_to_events), then
    events_to_voxel_torch on every slot's columns as float32; timed once, after one untimed pass, by host timers and a synchronise."""
    from bmc_hip import encodings
    pred = ms._bufs["pred"]

    def composition():
        xs, ys, ps, ts, index = encodings.counts_to_events(pred, ms.max_count, times="linear")
        for k in range(len(index) - 1):
            lo, hi = int(index[k]), int(index[k + 1])
            encodings.events_to_voxel_torch(xs[lo:hi].float(), ys[lo:hi].float(), ts[lo:hi].contiguous(), ps[lo:hi].float(),
                                            ms.voxel_bins, sensor_size=tuple(pred.shape[2:]))
        torch.cuda.synchronize()

    composition()
    t0 = time.perf_counter()
    composition()
    return 1e3 * (time.perf_counter() - t0)


RENDER_DIRS = {"lr": "lr_event_img", "bicubic": "hr_bicubic_event_img", "esr": "hr_esr_event_img", "gt": "hr_gt_event_img"}


def render_alone(ms):
    """{table: ms per bmc_slot_render call (select + colour)} on the session's buffers, for every render table the session's
    windows draw (Pictures.tables(): the table and count images of the last window; the repeated calls redraw the same pictures)."""
    from bmc_hip import slots
    part, b = ms.part(Pictures), ms._bufs
    return {name: alone(lambda: slots.render(b["table"], part.TABLES.index(name), h, w, rnd, b["render_minmax"]))
            for name, h, w, rnd in part.tables(ms)}


def write_images(root, name, images):
    """images {kind: uint8 [n,h,w,3]} of recording `name` -> root/name/event_img/<kind dir>/%09d.png (PIL): the arrays themselves."""
    from PIL import Image
    for kind, t in images.items():
        d = os.path.join(root, name, "event_img", RENDER_DIRS[kind])
        os.makedirs(d, exist_ok=True)
        for i, img in enumerate(t.cpu().numpy()):
            Image.fromarray(img, "RGB").save(os.path.join(d, "%09d.png" % i))


def sensor_spans(L, k, overlap=False):
    """Synthetic monotone float64 stamps of recording k: microseconds around 1e9, frame j spans [33 333 j, 33 333 j + 33 332];
    overlap: [33 333 j, 33 333 (j + 2) - 1] -- consecutive frames overlap by half, as the reference's blocks of 2 048 events
    that advance by 1 024."""
    import numpy as np
    t0 = 1e9 + 1e7 * k + 33333.0 * np.arange(L, dtype=np.float64)
    return np.stack([t0, t0 + (66665.0 if overlap else 33332.0)], 1)


def multistream(m, recs, S, graph, warmup, windows, events=False, emit=False, event_times=None, no_gt=False, clock=False,
                hot_filter=None, render=None, render_dir=None, voxel_bins=None, quality=None, overlap=False, continuous=False):
    ms = MultiStreamSR(m, S, n_c=128, scale=4, graph=graph, seqn=SEQN, emit_events=emit, event_times=event_times,
                       hot_filter=hot_filter, render=render, voxel_bins=voxel_bins, quality=quality, continuous=continuous)
    if events:
        dev = next(m.parameters()).device
        hs = [ms.open_events(tuple(t.to(dev) for t in r[0]), tuple(t.to(dev) for t in r[1]), *r[2:]) for r in recs[:S]]
    else:
        hs = [ms.open(f, None if no_gt else g, spans=sensor_spans(len(f), k, overlap) if clock else None)
              for k, (f, g) in enumerate(recs[:S])]
    for _ in range(warmup):
        ms.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(windows):
        ms.step()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    lat = statistics.median(ms.results(hs[0])["time"][warmup:])
    if emit:
        res = ms.results(hs[0])
        index = res["sr_index"]
        dense = MultiStreamSR(m, S, n_c=128, scale=4, seqn=SEQN, keep_predictions=True)
        stream = dict(events=int(index[-1]), dropped=sum(res.get("sr_dropped", ())), windows=len(index) - 1,      # of recording 0
                      sr_bytes=int(index[-1]) * sum(t.element_size() for t in res["sr_events"] + ((res["sr_ts"],) if "sr_ts" in res else ())))
        return (lat, S * windows / wall, part_alone(ms, EventStream), int(index[-1] - index[-2]), ms.resident_bytes(hs[0]),
                dense.resident_bytes(dense.open(*recs[0])), stream)
    if render:
        if render_dir:
            for k, h in enumerate(hs):
                write_images(render_dir, "rec%03d" % k, ms.results(h)["images"])
        return lat, S * windows / wall, render_alone(ms), ms.resident_bytes(hs[0])
    if voxel_bins is not None:
        return lat, S * windows / wall, part_alone(ms, VoxelGrids), voxel_composition(ms), ms.resident_bytes(hs[0])
    if quality is not None:
        return lat, S * windows / wall, part_alone(ms, Quality), quality_means(ms, hs), ms.resident_bytes(hs[0])
    if events:
        return lat, S * windows / wall, part_alone(ms, Input if hot_filter is None else HotFilter), ms.resident_bytes(hs[0])
    return lat, S * windows / wall, ms.resident_bytes(hs[0])


def quality_means(ms, hs):
    """{key: (mean over the recordings of the mean over a recording's finite windows, windows left out)} of the four quality keys."""
    import math
    out = {}
    for key in Quality.KEYS:
        per, skipped = [], 0
        for h in hs:
            v = ms.results(h)[key]
            finite = [x for x in v if math.isfinite(x)]
            skipped += len(v) - len(finite)
            if finite:
                per.append(statistics.mean(finite))
        out[key] = (statistics.mean(per) if per else float("nan"), skipped)
    return out


def structured_recording(L, H, W, seed, dev):
    """A synthetic recording with structure a super-resolver can use: the HR event rate is a field of drifting oriented bars
    (ON where they advance, OFF where they retreat), the ground truth its Poisson counts, an LR frame the Poisson counts of the
    4 x 4 block means -> (frames [L,2,H,W], gts [L,2,4H,4W]) on `dev`."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(4 * H, dtype=torch.float32), torch.arange(4 * W, dtype=torch.float32), indexing="ij")
    angle, period, speed = (torch.rand(3, generator=g) * torch.tensor([3.1416, 24.0, 3.0]) + torch.tensor([0.0, 12.0, 1.0])).tolist()
    phase = (xx * torch.cos(torch.tensor(angle)) + yy * torch.sin(torch.tensor(angle))) * (6.2832 / period)
    t = torch.arange(L, dtype=torch.float32)[:, None, None] * speed * (6.2832 / period)
    edge = torch.cos(phase[None] - t)                                      # the brightness change as the bars drift
    rate = torch.stack([edge.clamp(min=0), (-edge).clamp(min=0)], 1) ** 4 * 0.6 + 0.01
    gts = torch.poisson(rate, generator=g)
    frames = torch.poisson(torch.nn.functional.avg_pool2d(rate, 4), generator=g)
    return frames.to(dev), gts.to(dev)


def ensemble(m, plain, recs, S, K, graph, warmup, windows):
    """One session of S slots on the first S / (K or 1) recordings, self_ensemble=K (None: off) -> (ms per window, RECORDING
    windows per second, per recording the mean esr_mse and the mean bicubic_mse over its timed windows)."""
    ms = MultiStreamSR(m, S, n_c=128, scale=4, plain=plain, graph=graph, seqn=SEQN, self_ensemble=K)
    hs = [ms.open(f, g) for f, g in recs[:S // (K or 1)]]
    for _ in range(warmup):
        ms.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(windows):
        ms.step()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    res = [ms.results(h) for h in hs]
    mean = lambda key: [statistics.mean(r[key][warmup:]) for r in res]
    return statistics.median(res[0]["time"][warmup:]), len(hs) * windows / wall, mean("esr_mse"), mean("bicubic_mse")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="31x56,45x80,180x240")
    ap.add_argument("--slots", default="1,8,32")
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--events", action="store_true")
    ap.add_argument("--hot-filter", action="store_true",
                    help="implies --events: the event-backed session with the hot-pixel filter on and off, alternating runs")
    ap.add_argument("--noise-filter", default=None, metavar="DT[:K]",
                    help="implies --events: the event-backed session on recordings with a known share of uniform noise events, with "
                         "open_events(noise_filter=dict(ts=, dt=DT, support=K)) (DT in seconds of a one-second recording; K = 1) "
                         "and without, alternating runs: the share of events dropped and esr_mse of both")
    ap.add_argument("--from-hr", type=int, nargs="?", const=0, default=None, metavar="T",
                    help="adds the event-backed session on HR-only recordings (open_hr_events: the LR stream is synthesized on the "
                         "GPU by integrate-and-fire with threshold T, default scale^2) with PSNR / SSIM on")
    ap.add_argument("--runs", type=int, default=3, help="with --hot-filter / --noise-filter / --voxel-bins: alternating runs of each")
    ap.add_argument("--emit-events", action="store_true")
    ap.add_argument("--event-times", action="store_true",
                    help="with --emit-events: the timed, time-ordered stream (MultiStreamSR(event_times='linear'))")
    ap.add_argument("--sensor-clock", action="store_true",
                    help="implies --emit-events --event-times: float64 times on a synthetic sensor clock (spans= at open)")
    ap.add_argument("--continuous", action="store_true",
                    help="implies --sensor-clock: the synthetic spans overlap by half and the emitting session runs twice in this "
                         "process, with MultiStreamSR(continuous=True) and without -- window time and the six emit launches "
                         "alone of both, events kept / dropped and bytes of sr_* of a recording")
    ap.add_argument("--no-gt", action="store_true", help="adds the session on recordings without ground truth")
    ap.add_argument("--resident-windows", type=int, default=0)
    ap.add_argument("--modes", default="eager,graph")
    ap.add_argument("--out", default=None)
    ap.add_argument("--render", metavar="DIR", default=None,
                    help="adds the session with the event-count images on and writes them as DIR/<recording>/event_img/<kind dir>/"
                         "%%09d.png: the rendered arrays themselves (the reference's files are the same arrays resampled by "
                         "matplotlib at 300 dpi)")
    ap.add_argument("--render-kinds", default=None,
                    help="with --render: the kinds, a comma-separated choice of lr,bicubic,esr,gt (default: all four)")
    ap.add_argument("--voxel-bins", type=int, default=None, metavar="B",
                    help="adds the session with the per-window voxel grids on (voxel_bins=B, 1 .. 32) and off, alternating runs")
    ap.add_argument("--self-ensemble", type=int, default=None, metavar="K", choices=(2, 4, 8),
                    help="adds, per configuration whose slots K divides, the session with self_ensemble=K and the one without on the "
                         "same structured synthetic recordings: recording windows/s and mean esr_mse of both, --runs alternating runs")
    ap.add_argument("--plain-weights", metavar="NPZ", default=None,
                    help="with --self-ensemble: run BMCNet_plain(4,128,5) with the parameters of this file (p/<name> arrays, as "
                         "tests/golden/plain_pretrained_weights.npz) instead of a randomly initialised BMCNet")
    ap.add_argument("--quality", nargs="?", const="gt", default=None, metavar="RANGE",
                    help="adds the session with PSNR / SSIM on (quality=True; with a number: dict(data_range=RANGE)) and off, "
                         "alternating runs, and prints the recordings' means")
    a = ap.parse_args(argv)
    if a.quality is not None:
        try:
            a.quality = Quality.check("--quality: ", True if a.quality == "gt" else dict(data_range=float(a.quality)))
        except ValueError as e:
            ap.error(str(e))
    if a.plain_weights is not None and a.self_ensemble is None:
        ap.error("--plain-weights needs --self-ensemble K")
    if a.voxel_bins is not None and not 1 <= a.voxel_bins <= MultiStreamSR.MAX_VOXEL_BINS:
        ap.error("--voxel-bins: 1 <= B <= %d" % MultiStreamSR.MAX_VOXEL_BINS)
    if a.render_kinds is not None and a.render is None:
        ap.error("--render-kinds needs --render DIR")
    if a.render is not None:
        try:
            a.render_kinds = MultiStreamSR.check_render("--render-kinds: ", tuple(("lr,bicubic,esr,gt" if a.render_kinds is None else a.render_kinds).split(",")))
        except ValueError as e:
            ap.error(str(e))
    if a.continuous:
        a.sensor_clock = True
    if a.sensor_clock:
        a.emit_events = a.event_times = True
    if a.noise_filter is not None:
        from bmc_hip.encodings import check_noise_filter
        dt, _, k = a.noise_filter.partition(":")
        try:
            a.noise_filter = check_noise_filter("--noise-filter: ", dict(ts=torch.zeros(0, dtype=torch.float64), dt=float(dt), support=int(k or 1)))[1:]
        except ValueError as e:
            ap.error(str(e))
    if a.hot_filter or a.noise_filter is not None:
        a.events = True
    if a.event_times and not a.emit_events:
        ap.error("--event-times needs --emit-events")
    return a


def main():
    a = parse_args()
    render_dir = a.render
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = BMCNet(4, 128, 5).to(dev)
    em, eplain = m, False                                  # the model of the --self-ensemble rows
    if a.plain_weights is not None:
        import numpy as np
        from models.BMCNet_plain import BMCNet_plain
        em, eplain = BMCNet_plain(4, 128, 5), True
        z = np.load(a.plain_weights, allow_pickle=False)
        with torch.no_grad():
            for name, p in em.named_parameters():
                p.copy_(torch.from_numpy(z["p/" + name]))
        em.to(dev)
    rows = []
    L = a.warmup + a.windows + SEQN - 1 + int(a.continuous)   # (--continuous: one window more, so that every timed window has a cut)
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        g = torch.Generator().manual_seed(H * W)
        slots = [int(s) for s in a.slots.split(",")]
        recs = [(torch.poisson(torch.full((L, 2, H, W), 0.284), generator=g).to(dev),
                 torch.poisson(torch.full((L, 2, 4 * H, 4 * W), 0.1), generator=g).to(dev)) for _ in range(max(slots))]
        erecs = [event_recording(L, H, W, H * W + k) for k in range(max(slots))] if a.events else None
        nrecs = [noisy_event_recording(L, H, W, 3 * H * W + k) for k in range(max(slots))] if a.noise_filter is not None else None
        if a.resident_windows:
            r = event_recording(a.resident_windows + SEQN - 1, H, W, 1)
            r = (tuple(t.to(dev) for t in r[0]), tuple(t.to(dev) for t in r[1])) + r[2:]
            row = dict(size=size, runner="resident", windows=a.resident_windows)
            for key, kw in (("input_only", {}), ("dense_predictions", dict(keep_predictions=True)), ("event_output", dict(emit_events=True))):
                ms = MultiStreamSR(m, 1, n_c=128, scale=4, seqn=SEQN, **kw)
                row[key + "_bytes"] = ms.resident_bytes(ms.open_events(*r))
                del ms
                torch.cuda.empty_cache()
            rows.append(row)
            print(json.dumps(row), flush=True)
        for mode in a.modes.split(","):
            graph = mode == "graph"
            lat, wps = streaming(m, recs[0][0], graph, a.warmup, a.windows)
            rows.append(dict(size=size, mode=mode, runner="StreamingSR", slots=1, ms_per_window=round(lat, 3),
                             windows_per_s=round(wps, 1)))
            print(json.dumps(rows[-1]), flush=True)
            for S in slots:
                lat, wps, nbytes = multistream(m, recs, S, graph, a.warmup, a.windows)
                rows.append(dict(size=size, mode=mode, runner="MultiStreamSR", slots=S, ms_per_window=round(lat, 3),
                                 windows_per_s=round(wps, 1), resident_bytes=nbytes))
                print(json.dumps(rows[-1]), flush=True)
                if a.events:
                    lat, wps, enc, nbytes = multistream(m, erecs, S, graph, a.warmup, a.windows, events=True)
                    rows.append(dict(size=size, mode=mode, runner="MultiStreamSR(events)", slots=S, ms_per_window=round(lat, 3),
                                     windows_per_s=round(wps, 1), encode_ms=round(enc, 4), encode_share=round(enc / lat, 4),
                                     resident_bytes=nbytes))
                    print(json.dumps(rows[-1]), flush=True)
                if a.hot_filter:
                    off, on = [], []
                    for _ in range(a.runs):
                        off.append(multistream(m, erecs, S, graph, a.warmup, a.windows, events=True))
                        on.append(multistream(m, erecs, S, graph, a.warmup, a.windows, events=True, hot_filter=HOT_FILTER))
                    lat, upd = statistics.median(r[0] for r in on), statistics.median(r[2] for r in on)
                    rows.append(dict(size=size, mode=mode, runner="MultiStreamSR(events, hot filter)", slots=S, events=True,
                                     hot_filter=HOT_FILTER, ms_per_window=round(lat, 3),
                                     windows_per_s=round(statistics.median(r[1] for r in on), 1),
                                     windows_per_s_filter_off=round(statistics.median(r[1] for r in off), 1),
                                     windows_per_s_runs=[round(r[1], 1) for r in on],
                                     windows_per_s_filter_off_runs=[round(r[1], 1) for r in off],
                                     hot_update_alone_ms=round(upd, 4), hot_update_share=round(upd / lat, 4),
                                     resident_bytes=on[-1][3]))
                    print(json.dumps(rows[-1]), flush=True)
                if a.noise_filter is not None:
                    off, on = [], []
                    for _ in range(a.runs):
                        off.append(noise_session(m, nrecs, S, graph, a.warmup, a.windows, None))
                        on.append(noise_session(m, nrecs, S, graph, a.warmup, a.windows, a.noise_filter))
                    rows.append(dict(size=size, mode=mode, runner="MultiStreamSR(events, noise filter)", slots=S, events=True,
                                     noise_filter=dict(dt=a.noise_filter[0], support=a.noise_filter[1]),
                                     noise_share=round(sum(r[7] for r in nrecs[:S]) / sum(r[0][0].numel() for r in nrecs[:S]), 4),
                                     dropped_share=round(on[-1][3], 4), esr_mse=on[-1][2], esr_mse_filter_off=off[-1][2],
                                     ms_per_window=round(statistics.median(r[0] for r in on), 3),
                                     ms_per_window_filter_off=round(statistics.median(r[0] for r in off), 3),
                                     ms_per_window_runs=[round(r[0], 3) for r in on],
                                     ms_per_window_filter_off_runs=[round(r[0], 3) for r in off],
                                     windows_per_s=round(statistics.median(r[1] for r in on), 1),
                                     windows_per_s_filter_off=round(statistics.median(r[1] for r in off), 1)))
                    print(json.dumps(rows[-1]), flush=True)
                if a.from_hr is not None:
                    hrecs = [hr_recording(L, H, W, 5 * H * W + k) for k in range(S)]
                    lat, wps, made, door, mse, psnr, ssim = hr_session(m, hrecs, S, graph, a.warmup, a.windows, a.from_hr or None)
                    rows.append(dict(size=size, mode=mode, runner="MultiStreamSR(events, from HR)", slots=S, events=True,
                                     threshold=a.from_hr or 16, ms_per_window=round(lat, 3), windows_per_s=round(wps, 1),
                                     lr_events_per_hr_event=round(made, 5), open_hr_events_ms=round(door, 3), esr_mse=mse,
                                     esr_psnr=psnr, esr_ssim=ssim))
                    print(json.dumps(rows[-1]), flush=True)
                if a.render is not None:
                    lat, wps, alone, nbytes = multistream(m, recs, S, graph, a.warmup, a.windows, render=a.render_kinds,
                                                          render_dir=render_dir)
                    render_dir = None                      # (the first such session's images are the ones written)
                    rows.append(dict(size=size, mode=mode, runner="MultiStreamSR(render)", slots=S, kinds=list(a.render_kinds),
                                     ms_per_window=round(lat, 3), windows_per_s=round(wps, 1),
                                     render_ms={k: round(v, 4) for k, v in alone.items()},
                                     render_share=round(sum(alone.values()) / lat, 4), resident_bytes=nbytes))
                    print(json.dumps(rows[-1]), flush=True)
                if a.voxel_bins is not None:
                    off, on = [], []
                    for _ in range(a.runs):
                        off.append(multistream(m, recs, S, graph, a.warmup, a.windows))
                        on.append(multistream(m, recs, S, graph, a.warmup, a.windows, voxel_bins=a.voxel_bins))
                    lat, vox = statistics.median(r[0] for r in on), statistics.median(r[2] for r in on)
                    rows.append(dict(size=size, mode=mode, runner="MultiStreamSR(voxel)", slots=S, voxel_bins=a.voxel_bins,
                                     ms_per_window=round(lat, 3), windows_per_s=round(statistics.median(r[1] for r in on), 1),
                                     windows_per_s_voxel_off=round(statistics.median(r[1] for r in off), 1),
                                     windows_per_s_runs=[round(r[1], 1) for r in on],
                                     windows_per_s_voxel_off_runs=[round(r[1], 1) for r in off],
                                     voxel_alone_ms=round(vox, 4), voxel_share=round(vox / lat, 4),
                                     composition_ms=round(statistics.median(r[3] for r in on), 3), resident_bytes=on[-1][4]))
                    print(json.dumps(rows[-1]), flush=True)
                if a.quality is not None:
                    off, on = [], []
                    opt = True if a.quality == "gt" else dict(data_range=a.quality)
                    for _ in range(a.runs):
                        off.append(multistream(m, recs, S, graph, a.warmup, a.windows))
                        on.append(multistream(m, recs, S, graph, a.warmup, a.windows, quality=opt))
                    lat, qal = statistics.median(r[0] for r in on), statistics.median(r[2] for r in on)
                    rows.append(dict(size=size, mode=mode, runner="MultiStreamSR(quality)", slots=S, data_range=a.quality,
                                     ms_per_window=round(lat, 3), ms_per_window_quality_off=round(statistics.median(r[0] for r in off), 3),
                                     ms_per_window_runs=[round(r[0], 3) for r in on],
                                     ms_per_window_quality_off_runs=[round(r[0], 3) for r in off],
                                     windows_per_s=round(statistics.median(r[1] for r in on), 1),
                                     windows_per_s_quality_off=round(statistics.median(r[1] for r in off), 1),
                                     windows_per_s_runs=[round(r[1], 1) for r in on],
                                     windows_per_s_quality_off_runs=[round(r[1], 1) for r in off],
                                     quality_alone_ms=round(qal, 4), quality_share=round(qal / lat, 4),
                                     means={k: v[0] for k, v in on[-1][3].items()},
                                     nonfinite_windows={k: v[1] for k, v in on[-1][3].items()}, resident_bytes=on[-1][4]))
                    print(json.dumps(rows[-1]), flush=True)
                if a.self_ensemble is not None and S % a.self_ensemble == 0:
                    K = a.self_ensemble
                    srecs = [structured_recording(L, H, W, 7 * H * W + k, dev) for k in range(S)]
                    off, on = [], []
                    for _ in range(a.runs):
                        off.append(ensemble(em, eplain, srecs, S, None, graph, a.warmup, a.windows))
                        on.append(ensemble(em, eplain, srecs, S, K, graph, a.warmup, a.windows))
                    n = S // K                             # the recordings both sessions ran
                    rows.append(dict(size=size, mode=mode, runner="MultiStreamSR(self-ensemble)", slots=S, self_ensemble=K,
                                     model="BMCNet_plain, " + os.path.basename(a.plain_weights) if eplain else "BMCNet, random",
                                     ms_per_window=round(statistics.median(r[0] for r in on), 3),
                                     windows_per_s=round(statistics.median(r[1] for r in on), 1),
                                     windows_per_s_off=round(statistics.median(r[1] for r in off), 1),
                                     windows_per_s_runs=[round(r[1], 1) for r in on],
                                     windows_per_s_off_runs=[round(r[1], 1) for r in off],
                                     esr_mse=statistics.mean(on[-1][2]), esr_mse_off=statistics.mean(off[-1][2][:n]),
                                     bicubic_mse=statistics.mean(on[-1][3]), recordings=n))
                    print(json.dumps(rows[-1]), flush=True)
                    del srecs
                if a.no_gt:
                    lat, wps, nbytes = multistream(m, recs, S, graph, a.warmup, a.windows, no_gt=True)
                    rows.append(dict(size=size, mode=mode, runner="MultiStreamSR(no gt)", slots=S, ms_per_window=round(lat, 3),
                                     windows_per_s=round(wps, 1), resident_bytes=nbytes))
                    print(json.dumps(rows[-1]), flush=True)
                if a.emit_events:
                    lat, wps, emi, nev, nbytes, dense, stream = multistream(m, recs, S, graph, a.warmup, a.windows, emit=True,
                                                                            event_times="linear" if a.event_times else None,
                                                                            clock=a.sensor_clock, overlap=a.continuous)
                    rows.append(dict(size=size, mode=mode, runner="MultiStreamSR(emit, clocked)" if a.sensor_clock else
                                     "MultiStreamSR(emit, timed)" if a.event_times else "MultiStreamSR(emit)", slots=S, ms_per_window=round(lat, 3),
                                     windows_per_s=round(wps, 1), emit_ms=round(emi, 4), emit_share=round(emi / lat, 4),
                                     events_last_window=nev, resident_bytes=nbytes, resident_bytes_dense=dense))
                    if a.continuous:                       # the same spans with the option on, in this process
                        on = multistream(m, recs, S, graph, a.warmup, a.windows, emit=True, event_times="linear", clock=True,
                                         overlap=True, continuous=True)
                        rows[-1].update(runner="MultiStreamSR(emit, clocked | continuous)", ms_per_window_continuous=round(on[0], 3),
                                        windows_per_s_continuous=round(on[1], 1), emit_ms_continuous=round(on[2], 4),
                                        recording0_off=stream, recording0_continuous=on[6])
                    print(json.dumps(rows[-1]), flush=True)
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
