#!/usr/bin/env python3
"""Time the loss head of a window, fused against the chain it replaces, on the GPU: a ground truth that is not of the prediction's
size (train.py:227-231) and, for the equal-size path, BASELINE's C2 frame.

--loss mse|l1|huber:DELTA|charbonnier:EPS|ssim[:R]|POINT+ssim[:R][@ALPHA] (default mse) picks the loss; fused and unfused
evaluate the SAME loss object (unfused: the object's plain-torch __call__, for ssim a float64 chain of avg_pool2d and elementwise ops).
Part `isolated`: forward + backward of the head and loss alone, with a gradient arriving from the next window as in a BPTT step,
  fused    ops.loss_head: mse -> ops.head_mse / ops.head_resize_mse (bmc_head_mse_* / bmc_head_resize_mse_*), a pointwise loss ->
           bmc_head_loss_fwd / _bwd, ssim -> ops.head, ops.bicubic_resize, ops.ssim_loss (bmc_ssim_loss_fwd / _bwd), a mix -> the
           pointwise head plus ops.ssim_loss on its prediction
  unfused  the composition it replaces: ops.head -> ops.bicubic_resize (where the sizes differ) -> the loss in torch ops,
           autograd's backward of the three and its add of the two gradients that reach the prediction
at LR 31x56 -> 124x222 (EventZoom), LR 65x87 -> 260x346 (DAVIS346) and LR 180x240 -> 720x960 (C2: the prediction's own size, no
resize on either side), B = 4, x4.  Each timed repetition is --inner back-to-back
calls between two device events (the launches are tens of microseconds; one call is below what a pair of events resolves).
Part `step`: the whole train_step.bptt_step of BMCNet(4,128,5) at BASELINE configs[3]'s shape (31x56, B = 4, L = 9), in fp32 and bf16,
  fused    ground truth 124x222, loss_fn = F.mse_loss or the bmc_hip.losses object
  unfused  ground truth 124x222, the unfused chain selected through a lambda around the same loss
  same     ground truth 124x224 (the synthetic size bench.py times)
Part `ssim` (structural losses only): the loss ALONE on a prediction of the ground truth's size -- forward (under no_grad) and
backward (of a retained graph) timed separately, the device path (the loss object's structural term through ops.ssim_loss, a mix's
pointwise term in torch ops on both sides) against the object's plain-torch form, with the kernel launches of one forward and one
backward of each counted by torch.profiler -- at the reference's training shape (180x320, B = 2) and C2 (720x960, B = 4).
The variants alternate inside one process, every variant is warmed before anything is timed, a repetition ends in a device
synchronise; reported: median and range over --reps (>= 15) repetitions, every repetition in the JSON, and fused / unfused per
repetition (they run back to back; the launches are host-issue-bound and the host's speed changes under other people's work).
No GPU is an error: nothing here runs on the CPU.

python tools/time_head_loss.py [--part isolated|step|ssim|all] [--variants fused,unfused,same] [--reps 15] [--inner 50] [--warmup 3]
                               [--math fp32,bf16] [--loss mse] [--out FILE]
For a launch count, trace one variant at a time:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_head_loss.py
--part isolated --variants fused --reps 1 --inner 1 --warmup 0 --allow-few-reps   (then the same with --variants unfused).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bmcnet-esr_amd")]
import torch
import torch.nn.functional as F

ISOLATED = [("EventZoom", 31, 56, 124, 222), ("DAVIS346", 65, 87, 260, 346), ("C2", 180, 240, 720, 960)]
SCALE, B, L, N_C, N_B = 4, 4, 9, 128, 5


def timed(fn, inner):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(inner):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / inner


def alternate(variants, reps, inner, warmup):
    """{name: fn} -> {name: [ms per call] * reps}, one repetition of every variant in turn, after `warmup` untimed
    repetitions of every variant (the same `inner` calls each)."""
    for _ in range(warmup):
        for fn in variants.values():
            timed(fn, inner)
    out = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            out[k].append(timed(fn, inner))
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5), "reps": len(ms),
            "all_ms": [round(v, 5) for v in ms]}


def paired(tag, ms, row):
    """fused / unfused per repetition: the two were timed back to back, so a change of the host's speed between repetitions
    (these launches are host-issue-bound, and the host is shared) moves both and leaves the ratio."""
    if "fused" in ms and "unfused" in ms:
        q = [f / u for f, u in zip(ms["fused"], ms["unfused"])]
        row["fused_over_unfused"] = {"median": round(statistics.median(q), 4), "min": round(min(q), 4), "max": round(max(q), 4)}
        print("%s fused / unfused per repetition: %.3f  (%.3f .. %.3f)" % (tag, statistics.median(q), min(q), max(q)), flush=True)


def isolated(dev, want, reps, inner, warmup, loss):
    from bmc_hip import ops
    loss_fn = F.mse_loss if loss is None else loss
    rows = {}
    for name, H, W, gh, gw in ISOLATED:
        torch.manual_seed(0)
        xo = torch.randn(B, H, W, 2 * SCALE * SCALE, device=dev, requires_grad=True)
        base = torch.poisson(torch.full((B, 2, 3, H, W), 0.3)).to(dev)[:, :, 1]       # frame 1 of the window, as the model passes it
        gt = torch.poisson(torch.full((B, 2, gh, gw), 0.3)).to(dev)
        dpred = torch.randn(B, 2, SCALE * H, SCALE * W, device=dev)
        one = torch.ones((), device=dev)

        def fused():
            pred, mse = ops.loss_head(xo, base, gt, SCALE, loss)
            return torch.autograd.grad([pred, mse], [xo], [dpred, one])[0]

        def unfused():
            pred = ops.head(xo, base, SCALE)
            mse = loss_fn(ops.bicubic_resize(pred, (gh, gw)), gt)
            return torch.autograd.grad([pred, mse], [xo], [dpred, one])[0]

        variants = {k: f for k, f in (("fused", fused), ("unfused", unfused)) if k in want}
        ms = alternate(variants, reps, inner, warmup)
        rows[name] = {"shape": "LR %dx%d -> %dx%d, B=%d, x%d" % (H, W, gh, gw, B, SCALE), "inner": inner,
                      **{k: summary(v) for k, v in ms.items()}}
        if len(variants) == 2:                                        # the two must be the same function of their operands
            a, b = fused(), unfused()
            rows[name]["max_abs_grad_difference"] = float((a - b).abs().max())
        for k, v in ms.items():
            s = rows[name][k]
            print("isolated %-9s %-8s %9.2f us  (%.2f .. %.2f, %d reps x %d calls)" % (name, k, s["median_ms"] * 1e3, s["min_ms"] * 1e3,
                                                                                 s["max_ms"] * 1e3, s["reps"], inner), flush=True)
        paired("isolated %-9s" % name, ms, rows[name])
    return rows


SSIM_SHAPES = [("train", 2, 180, 320), ("C2", 4, 720, 960)]


def launches(fn):
    """Kernel launches of one call of fn, counted by torch.profiler (None where the profiler reports no device activity)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and
            "memset" not in e.name.lower())
    return n or None


def ssim_alone(dev, want, reps, inner, warmup, loss):
    from bmc_hip import losses, ops
    structural = loss if isinstance(loss, losses.SSIM) else loss.structural

    def device(pred, gt):
        s = ops.ssim_loss(pred, gt, structural.param)
        if structural is loss:
            return s
        point = F.mse_loss(pred, gt) if loss.pointwise is None else loss.pointwise(pred, gt)
        return (1.0 - loss.alpha) * point + loss.alpha * s

    rows = {}
    for name, b, h, w in SSIM_SHAPES:
        torch.manual_seed(0)
        gt = torch.poisson(torch.full((b, 2, h, w), 0.3)).to(dev)
        pred = (gt + 0.5 * torch.randn_like(gt)).requires_grad_()
        paths = {k: f for k, f in (("fused", device), ("unfused", lambda a, g: loss(a, g))) if k in want}
        row = rows[name] = {"shape": "%dx%d, B=%d" % (h, w, b), "inner": inner}

        def fwd(f):
            def run():
                with torch.no_grad():
                    f(pred, gt)
            return run

        held = {k: f(pred, gt) for k, f in paths.items()}
        bwd = lambda k: (lambda: torch.autograd.grad(held[k], pred, retain_graph=True))
        for tag, variants in (("forward", {k: fwd(f) for k, f in paths.items()}), ("backward", {k: bwd(k) for k in paths})):
            ms = alternate(variants, reps, inner, warmup)
            row[tag] = {k: summary(v) for k, v in ms.items()}
            for k in ms:
                s = row[tag][k]
                row[tag][k]["launches"] = launches(variants[k])
                print("ssim %-5s %-8s %-8s %9.2f us  (%.2f .. %.2f, %d reps x %d calls)  launches %s" % (
                    name, tag, k, s["median_ms"] * 1e3, s["min_ms"] * 1e3, s["max_ms"] * 1e3, s["reps"], inner, s["launches"]), flush=True)
            paired("ssim %-5s %-8s" % (name, tag), ms, row[tag])
        if len(paths) == 2:
            row["loss_difference"] = abs(float(held["fused"]) - float(held["unfused"]))
            row["max_abs_grad_difference"] = float((bwd("fused")()[0] - bwd("unfused")()[0]).abs().max())
    return rows


def step(dev, want, maths, reps, warmup, loss):
    from bmc_hip import ops
    from models.BMCNet import BMCNet
    from train_step import bptt_step
    H, W = 31, 56
    rows = {}
    for math in maths:
        ops.set_math(math)
        torch.manual_seed(3407)
        m = BMCNet(SCALE, N_C, N_B).to(dev)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=1e-5, amsgrad=True)
        inp = torch.poisson(torch.full((B, L, 2, H, W), 0.57)).to(dev)
        gt222 = torch.poisson(torch.full((B, L, 2, 124, 222), 0.57)).to(dev)
        gt224 = torch.poisson(torch.full((B, L, 2, 124, 224), 0.57)).to(dev)
        loss_fn = F.mse_loss if loss is None else loss
        wrapped = lambda a, b: loss_fn(a, b)
        all_v = {"fused": lambda: bptt_step(m, opt, inp, gt222, N_C, SCALE, loss_fn=loss_fn),
                 "unfused": lambda: bptt_step(m, opt, inp, gt222, N_C, SCALE, loss_fn=wrapped),
                 "same": lambda: bptt_step(m, opt, inp, gt224, N_C, SCALE, loss_fn=loss_fn)}
        variants = {k: f for k, f in all_v.items() if k in want}
        ms = alternate(variants, reps, 1, warmup)
        rows[math] = {"shape": "BMCNet(4,128,5) bptt_step, LR %dx%d, B=%d, L=%d, %s" % (H, W, B, L, math),
                      **{k: summary(v) for k, v in ms.items()}}
        for k in ms:
            s = rows[math][k]
            print("step %-5s %-8s %9.3f ms  (%.3f .. %.3f, %d reps)" % (math, k, s["median_ms"], s["min_ms"], s["max_ms"], s["reps"]),
                  flush=True)
        paired("step %-5s" % math, ms, rows[math])
    ops.set_math("fp32")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("isolated", "step", "ssim", "all"), default="all")
    ap.add_argument("--variants", default="fused,unfused,same")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--math", default="fp32,bf16")
    ap.add_argument("--allow-few-reps", action="store_true", help="for a kernel trace: fewer than 15 repetitions, no timing claimed")
    ap.add_argument("--loss", default="mse", help="mse | l1 | huber:DELTA | charbonnier:EPS | ssim[:R] | POINT+ssim[:R][@ALPHA]")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from bmc_hip import losses
    try:
        loss = losses.parse(a.loss)                                   # None: nn.MSELoss
    except ValueError as e:
        ap.error("--loss: %s" % e)
    if a.reps < 15 and not a.allow_few_reps:
        ap.error("a timing needs at least 15 repetitions per variant (--allow-few-reps for a kernel trace)")
    if not torch.cuda.is_available():
        raise SystemExit("time_head_loss: no GPU -- these are GPU timings, nothing falls back to the CPU")
    dev = torch.device("cuda:0")
    want = set(a.variants.split(","))
    out = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "warmup": a.warmup, "loss": a.loss}
    if a.part in ("isolated", "all"):
        out["isolated"] = isolated(dev, want, a.reps, a.inner, a.warmup, loss)
    if a.part in ("ssim", "all") and losses.is_structural(loss):
        out["ssim"] = ssim_alone(dev, want, a.reps, a.inner, a.warmup, loss)
    elif a.part == "ssim":
        ap.error("--part ssim times a structural loss: --loss ssim[:R] or POINT+ssim[:R][@ALPHA]")
    if a.part in ("step", "all"):
        out["step"] = step(dev, want, a.math.split(","), a.reps, a.warmup, loss)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
