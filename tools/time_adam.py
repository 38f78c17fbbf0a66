#!/usr/bin/env python3
"""The optimizer step alone: torch.optim.Adam with its default (foreach), torch.optim.Adam(foreach=False) and
bmc_hip.optim.Adam (csrc/optim.hip, ONE launch) on the BMCNet(4,128,5) and BMCNet_plain(4,128,5) parameter sets with random
gradients, Adam(lr=1e-4, weight_decay=1e-5, amsgrad=True) as train.py:653 builds it.

Timing: the three optimizers alternate in one process, HIP events around --steps steps after --warmup steps, --rounds rounds
each; every round is printed (ms per step: the GPU-side span of the step's launches as the host issues them, so a host that
cannot keep up shows here too) and the median.  Floors for comparison: 36 bytes per element over 6.3 TB/s of HBM.

--trace: the kernel launches per step.  Each optimizer runs twice in a child process of its own under
`rocprofv3 --kernel-trace --stats -- python tools/time_adam.py --only NAME --steps N` (N = 2 and N = 7, no timing) and the
difference of the two traces' kernel counts over 5 steps is printed: set-up kernels cancel.  No counters are collected.

--clip: the clipped step (csrc/optim.hip as well, TWO launches).  Three figures per set: hip_clip, bmc_hip.optim.Adam(max_grad_norm=
--clip-norm); hip, the unclipped fused step (the difference is the cost of the feature); foreach_clip, what a user has otherwise:
torch.nn.utils.clip_grad_norm_ with its default foreach followed by torch.optim.Adam with its default.  Floor of the clipped step:
40 bytes per element (the norm launch reads g once more) and one more launch.

--ema DECAY: the weight EMA inside the step (csrc/optim_ema.hip).  Three figures per set, each with the host's wall time per step
(perf_counter around the loop that issues the steps, before the device is waited for): hip_ema, bmc_hip.optim.Adam(ema_decay=DECAY)
(with --clip also max_grad_norm); hip, the same optimizer without the option (44 against 36 bytes per element); hip_swa, what a user
has otherwise: torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(DECAY)).update_parameters() after
bmc_hip.optim.Adam.step().  Then the exchange launch alone (bmc_ema_swap, 16 bytes per element).

python tools/time_adam.py [--steps 50 --warmup 10 --rounds 3] [--sets bmcnet,plain] [--only NAME] [--clip [--clip-norm 1.0]]
                          [--trace [--trace-dir DIR]] [--ema DECAY]
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bmcnet-esr_amd")]

CFG = dict(lr=1e-4, weight_decay=1e-5, amsgrad=True)
NAMES = ("foreach", "single", "hip")
CLIP_NAMES = ("foreach_clip", "hip", "hip_clip")
EMA_NAMES = ("hip_swa", "hip", "hip_ema")


class TorchClipped:
    """clip_grad_norm_ (default foreach) and torch.optim.Adam (default foreach) as one step()"""

    def __init__(self, params, max_norm):
        import torch
        self.params, self.max_norm, self.opt = params, max_norm, torch.optim.Adam(params, **CFG)

    def step(self):
        import torch
        torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
        self.opt.step()


class HipWithAveragedModel:
    """bmc_hip.optim.Adam.step() followed by torch's AveragedModel update: a second copy of the weights and a foreach pass"""

    def __init__(self, params, decay, **kw):
        import torch
        from bmc_hip.optim import Adam
        from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
        self.opt = Adam(params, **CFG, **kw)
        self.model = torch.nn.Module()
        self.model.w = torch.nn.ParameterList(params)
        self.avg = AveragedModel(self.model, multi_avg_fn=get_ema_multi_avg_fn(decay))

    def step(self):
        self.opt.step()
        self.avg.update_parameters(self.model)


def make(name, params, clip_norm=1.0, ema=None, clip=False):
    import torch
    from bmc_hip.optim import Adam
    if ema is not None:                          # the three variants of --ema, clipped alike with --clip
        kw = dict(max_grad_norm=clip_norm) if clip else {}
        if name == "hip_ema":
            return Adam(params, ema_decay=ema, **kw, **CFG)
        if name == "hip_swa":
            return HipWithAveragedModel(params, ema, **kw)
        return Adam(params, **kw, **CFG)
    if name == "hip":
        return Adam(params, **CFG)
    if name == "hip_clip":
        return Adam(params, max_grad_norm=clip_norm, **CFG)
    if name == "foreach_clip":
        return TorchClipped(params, clip_norm)
    return torch.optim.Adam(params, foreach=None if name == "foreach" else False, **CFG)


def parameter_set(kind, dev):
    import torch
    from models.BMCNet import BMCNet
    from models.BMCNet_plain import BMCNet_plain
    torch.manual_seed(0)
    model = (BMCNet if kind == "bmcnet" else BMCNet_plain)(4, 128, 5)
    params = [torch.nn.Parameter(p.detach().to(dev)) for p in model.parameters()]
    gen = torch.Generator().manual_seed(1)
    for p in params:
        p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(dev)
    return params


def timed(opt, steps, wall=None):
    import time
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.step()
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    if wall is not None:
        wall.append((t1 - t0) * 1e3 / steps)     # the host's share: issuing the steps, not waiting for them
    return e0.elapsed_time(e1) / steps


class Swapper:
    """step() is one exchange of parameters and averages (bmc_ema_swap); an even number of them leaves everything as it was"""

    def __init__(self, opt):
        self.step = opt._swap


def run(a):
    import torch
    dev = torch.device("cuda:0")
    made = [a.only] if a.only else list(EMA_NAMES if a.ema is not None else CLIP_NAMES if a.clip else NAMES)
    for kind in a.sets.split(","):
        base = parameter_set(kind, dev)
        n = sum(p.numel() for p in base)
        opts = {}
        names = list(made)
        for name in names:                      # every optimizer on its own copy of the parameters, the same gradients
            params = [torch.nn.Parameter(p.detach().clone()) for p in base]
            for p, q in zip(params, base):
                p.grad = q.grad.clone()
            opts[name] = make(name, params, a.clip_norm, a.ema, a.clip)
        if a.ema is not None and "hip_ema" in opts:
            names = names + ["swap"]
            opts["swap"] = Swapper(opts["hip_ema"])
        for _ in range(a.warmup + a.warmup % 2):     # (an even count: the exchange is its own inverse)
            for name in names:
                opts[name].step()
        torch.cuda.synchronize()
        if a.rounds == 0:                       # the traced runs: the steps, no timing
            for name in names:
                for _ in range(a.steps):
                    opts[name].step()
            torch.cuda.synchronize()
            continue
        rounds = {name: [] for name in names}
        walls = {name: [] for name in names}
        for _ in range(a.rounds):
            for name in names:                  # alternating: what shares the machine hits all three alike
                rounds[name].append(timed(opts[name], a.steps + (a.steps % 2 if name == "swap" else 0), walls[name]))
        per = (40 if a.clip else 36) + (8 if a.ema is not None else 0)
        print("%s: %d tensors, %d elements, %.1f MB per pass (%d B per element; %.1f us at 6.3 TB/s)" % (
            kind, len(base), n, per * n / 1e6, per, per * n / 6.3e12 * 1e6))
        for name in names:
            print("  %-12s ms per step, %d steps per round: %s   median %.4f" % (
                name, a.steps, "  ".join("%.4f" % v for v in rounds[name]), statistics.median(rounds[name])) +
                ("   host wall %.4f" % statistics.median(walls[name]) if a.ema is not None else ""))


def kernel_count(out_dir):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel trace under %s" % out_dir)
    total = 0
    for f in files:
        with open(f, newline="") as fh:
            total += sum(1 for _ in csv.DictReader(fh))
    return total


def trace(a):
    base = a.trace_dir or tempfile.mkdtemp(prefix="time_adam_trace_")
    for kind in a.sets.split(","):
        for name in ([a.only] if a.only else (CLIP_NAMES if a.clip else NAMES)):
            counts = {}
            for steps in (2, 7):
                out = os.path.join(base, "%s_%s_%d" % (kind, name, steps))
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "t", "--", sys.executable,
                       os.path.abspath(__file__), "--only", name, "--clip-norm", str(a.clip_norm), "--sets", kind, "--steps", str(steps), "--warmup", "0", "--rounds", "0"]
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.child_timeout)
                if r.returncode != 0:
                    raise SystemExit("traced run failed (rc %d):\n%s" % (r.returncode, r.stdout.decode()[-2000:]))
                counts[steps] = kernel_count(out)
            print("%s %-8s kernel launches per step: %.1f   (%d kernels in 7 steps, %d in 2)" % (
                kind, name, (counts[7] - counts[2]) / 5.0, counts[7], counts[2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", default="bmcnet,plain")
    ap.add_argument("--only", choices=NAMES + CLIP_NAMES[::2] + EMA_NAMES[::2], default=None)
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY")
    ap.add_argument("--clip", action="store_true")
    ap.add_argument("--clip-norm", type=float, default=1.0)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-dir", default=None)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    a = ap.parse_args()
    if a.ema is None and a.only in ("hip_swa", "hip_ema"):
        ap.error("--only %s needs --ema DECAY" % a.only)
    if a.ema is not None and a.trace:
        ap.error("--ema is timed, not traced: no launch is added to the step")
    if a.trace:
        trace(a)           # this process never opens the GPU: each traced run is a fresh child
    else:
        run(a)


if __name__ == "__main__":
    main()
