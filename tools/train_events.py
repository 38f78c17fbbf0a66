#!/usr/bin/env python3
"""Train from recordings kept on the GPU as raw event columns (event_dataset.EventTrainSet): N bptt_steps whose batches are
encoded by ONE bmc_seq_encode launch each; prints the loss per step and the encode time per batch (HIP events around
EventTrainSet.batch's launch: the table copy and the kernel).

A recording is an .npz of raw columns, the ones tools/multistream_infer.py --events builds synthetically (event_recording):
lr_xs / lr_ys (int16), lr_ps (float64), lr_ts (float64, sorted), the same four with gt_, and lr_size = (H, W), gt_size = (gh, gw).
The index tables are cut here with bmc_hip.encodings.event_window_indices (the reference's blocks: --window / --sliding).
--synthetic K makes K such recordings of --items items at --size instead (and --save DIR writes them out); --gt-size HxW gives
them a ground truth that is not scale x LR (EventZoom: --size 31x56 --gt-size 124x222), so every window takes the bicubic
branch of train.py:227-231 -- inside bptt_step's fused head + loss launches.

python tools/train_events.py [rec.npz ...] [--synthetic 2 --items 24 --size 45x80] [--steps 10] [--batch 2] [--L 9] [--step-size S]
                             [--augment] [--pause 0.05,0.9] [--noise 0.01] [--n-c 128 --n-b 5] [--seed 0] [--out FILE]
                             [--optimizer hip|torch] [--clip-norm X] [--nonfinite propagate|skip] [--wall]
                             [--gt-size HxW] [--valid-every N] [--crop HxW] [--transpose [P]]
                             [--loss mse|l1|huber:DELTA|charbonnier:EPS|ssim[:R]|POINT+ssim[:R][@ALPHA]] [--ema DECAY [--ema-warmup] [--save-ema PATH]]
--ema DECAY (hip only): Adam(ema_decay=DECAY), an exponential moving average of the weights kept inside the step launch
(csrc/optim_ema.hip); --ema-warmup ramps the decay as min(DECAY, t / (t + 9)).  With --valid-every the held-out sequences are
also run under opt.ema_weights() and `valid_loss_ema` is printed beside `valid_loss`.  --save-ema PATH writes
opt.ema_state_dict(model) there at the end, a bare checkpoint for checkpoint.load_model_state (--save is taken: it names the
directory of the synthetic recordings).
--loss: the training (and validation) loss, default mse (nn.MSELoss, the reference's).  l1, huber:DELTA (default 1) and
charbonnier:EPS (default 1e-3) are bmc_hip.losses objects: the same fused head + loss launches with another pointwise function,
at either ground-truth size.  ssim[:R] is 1 - mean SSIM with the constant data range R (default 1, one event; bmc_hip.losses.SSIM)
and POINT+ssim[:R][@ALPHA], POINT one of mse | l1 | huber[:D] | charbonnier[:E], the mix (1 - ALPHA) POINT + ALPHA ssim (default
0.84; l1+ssim:8@0.84): the pointwise term stays on the fused head, the structural one runs bmc_ssim_loss_fwd / _bwd on its prediction.
--crop HxW: train on HxW LR patches (and scale x that HR patches) cut in the encoder, one random origin per sequence
(EventTrainSet(crop=...), ONE bmc_seq_encode_crop launch per batch).  --size and --gt-size then take comma-separated lists the
synthetic recordings cycle through (--size 180x240,260x346), a set of mixed sensors; recordings given as files may differ in size
too.  Validation stays on full frames.
--transpose [P]: with --crop, "Transpose" joins the augmentation at probability P (0.5): a sample that draws it is the patch of
its transposed frames, cut in the same launch -- with --augment's flips, all 8 orientations of a patch.  It implies no flips;
the patch must fit every recording both ways.  Validation stays on untransposed full frames.
--denoise DT[:K]: every training recording is added with noise_filter=dict(ts=its LR timestamps, dt=DT, support=K) (K = 1): the
background-activity filter of include/bmc_hip_denoise.h runs once per recording, on the GPU, and the LR events it drops train with
weight zero; the events dropped are printed.  DT is in the units of the recordings' timestamps.  The held-out recording of
--valid-every is filtered too; the ground truth never is.
--from-hr [T]: the recordings' LR halves are not read: every recording is added with EventTrainSet.add_hr_recording, which makes
the LR stream from the HR one on the GPU by integrate-and-fire over scale x scale blocks (include/bmc_hip_downsample.h; threshold T,
default scale^2) and cuts both index tables from the synthetic timestamps; the LR events made are printed.  With --denoise the
filter acts on the synthetic LR stream.  Uniform random events fire rarely (a random walk needs about T^2 steps to reach T): give
the synthetic recordings of this tool a small T, or real recordings.
--valid-every N: the last recording is held out of training; after every N steps train_step.valid_step (the reference's _valid
loop: eval mode, no gradients, the same loss) runs over its sequences in order and `valid_loss`, their mean, is printed.
--optimizer: hip (default) steps with bmc_hip.optim.Adam (csrc/optim.hip, one launch per step), torch with torch.optim.Adam.
--clip-norm X: clip the gradients by their global L2 norm.  hip: Adam(max_grad_norm=X), a norm launch and a step launch
(csrc/optim.hip); torch: torch.nn.utils.clip_grad_norm_ in a pre-step hook, so that the two can be compared.
--nonfinite skip (hip only): a step whose gradients hold an Inf or a NaN leaves parameters and state untouched.
With either, the norm and coefficient of the last step and the number of skipped steps are printed once at the end.
--wall: also print the wall time per step at the end (host clock, device synchronised, the first step left out).
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bmcnet-esr_amd")]
import numpy as np
import torch

from bmc_hip import losses
from bmc_hip.encodings import check_noise_filter, event_window_indices
from event_dataset import EventTrainSet
from models.BMCNet import BMCNet
from train_step import bptt_step, valid_step

KEYS = ("xs", "ys", "ps", "ts")


def synthetic_recording(items, H, W, scale, window, sliding, seed, gt_size=None):
    """Raw columns of about `items` items: uniform coordinates, +-1 polarities, sorted uniform timestamps.  gt_size: the
    ground truth's (gh, gw) where it is not (scale H, scale W)."""
    rng = np.random.default_rng(seed)
    n_lr = (window - sliding) * items + 1
    gh, gw = gt_size or (scale * H, scale * W)
    rec = {"lr_size": np.asarray([H, W]), "gt_size": np.asarray([gh, gw])}
    for side, n, h, w in (("lr", n_lr, H, W), ("gt", scale * scale * n_lr, gh, gw)):
        rec[side + "_xs"] = rng.integers(0, w, n).astype(np.int16)
        rec[side + "_ys"] = rng.integers(0, h, n).astype(np.int16)
        rec[side + "_ps"] = rng.choice([-1.0, 1.0], n)
        rec[side + "_ts"] = np.sort(rng.uniform(0, 1, n))
    return rec


def add(ts, rec, dev, window, sliding, scale, denoise=None, from_hr=None):
    cols = lambda side: tuple(torch.from_numpy(np.ascontiguousarray(rec["%s_%s" % (side, k)])).to(dev) for k in KEYS[:3])
    if from_hr is not None:
        nf = None if denoise is None else dict(dt=denoise[0], support=denoise[1])
        gt_ts = torch.from_numpy(np.ascontiguousarray(rec["gt_ts"], np.float64)).to(dev)
        k = ts.add_hr_recording(cols("gt"), gt_ts, tuple(rec["gt_size"].tolist()), window, sliding, threshold=from_hr or None,
                                noise_filter=nf)
        print("recording %d: %d LR events synthesized from %d HR events" % (k, ts.synthesized_events(k), len(rec["gt_xs"])))
        return k
    lr_index, gt_index = event_window_indices(rec["lr_ts"], rec["gt_ts"], window, sliding, scale)
    nf = None
    if denoise is not None:
        nf = dict(ts=torch.from_numpy(np.ascontiguousarray(rec["lr_ts"], np.float64)).to(dev), dt=denoise[0], support=denoise[1])
    return ts.add_recording(cols("lr"), cols("gt"), lr_index, gt_index, tuple(rec["lr_size"].tolist()), tuple(rec["gt_size"].tolist()),
                            noise_filter=nf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("recordings", nargs="*")
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--items", type=int, default=24)
    ap.add_argument("--size", default="45x80")
    ap.add_argument("--save", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--L", type=int, default=9)
    ap.add_argument("--step-size", type=int, default=None)
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--sliding", type=int, default=1024)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--augment", action="store_true", help="Horizontal / Vertical / Polarity flips, 0.5 each")
    ap.add_argument("--pause", default=None, help="proba_pause_when_running,proba_pause_when_paused")
    ap.add_argument("--noise", type=float, default=None, help="noise_level")
    ap.add_argument("--n-c", type=int, default=128)
    ap.add_argument("--n-b", type=int, default=5)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--optimizer", choices=("hip", "torch"), default="hip")
    ap.add_argument("--clip-norm", type=float, default=None)
    ap.add_argument("--nonfinite", choices=("propagate", "skip"), default="propagate")
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--gt-size", default=None, help="HxW of the synthetic recordings' ground truth (default: scale x --size)")
    ap.add_argument("--valid-every", type=int, default=0, help="hold the last recording out and print valid_loss every N steps")
    ap.add_argument("--crop", default=None, help="HxW of the LR patches to train on; --size / --gt-size may then be lists")
    ap.add_argument("--transpose", type=float, nargs="?", const=0.5, default=None, metavar="P",
                    help="with --crop: transpose a sample's frames with probability P (default 0.5)")
    ap.add_argument("--loss", default="mse", help="mse | l1 | huber:DELTA | charbonnier:EPS | ssim[:R] | POINT+ssim[:R][@ALPHA]")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY", help="keep an EMA of the weights inside the step (hip only)")
    ap.add_argument("--ema-warmup", action="store_true", help="decay_t = min(DECAY, t / (t + 9))")
    ap.add_argument("--save-ema", default=None, metavar="PATH", help="write the EMA weights there at the end (a bare state_dict)")
    ap.add_argument("--denoise", default=None, metavar="DT[:K]",
                    help="filter the LR streams: drop events with fewer than K (1) neighbour pixels active within DT before them")
    ap.add_argument("--from-hr", type=int, nargs="?", const=0, default=None, metavar="T",
                    help="make every recording's LR stream from its HR stream on the GPU (integrate-and-fire, threshold T = scale^2)")
    a = ap.parse_args()
    try:
        loss_obj = losses.parse(a.loss)                       # None: nn.MSELoss
    except ValueError as e:
        ap.error("--loss: %s" % e)
    denoise = None
    if a.denoise is not None:
        dt, _, k = a.denoise.partition(":")
        try:
            denoise = check_noise_filter("--denoise: ", dict(ts=torch.zeros(0, dtype=torch.float64), dt=float(dt), support=int(k or 1)))[1:]
        except ValueError as e:
            ap.error(str(e))
    if not a.recordings and not a.synthetic:
        ap.error("give recordings or --synthetic K")
    if a.ema is None and (a.ema_warmup or a.save_ema):
        ap.error("--ema-warmup and --save-ema need --ema DECAY")
    if a.ema is not None and a.optimizer != "hip":
        ap.error("--ema needs --optimizer hip (the average is kept by the fused step)")
    if a.transpose is not None and not a.crop:
        ap.error("--transpose needs --crop: full frames of one size cannot hold a transposed sample")
    dev = torch.device("cuda:0")
    hw = lambda text: tuple(int(v) for v in text.split("x"))
    sizes = [hw(t) for t in a.size.split(",")]
    gt_sizes = [hw(t) for t in a.gt_size.split(",")] if a.gt_size else [None]
    crop = hw(a.crop) if a.crop else None
    if crop is None and (len(sizes) > 1 or len(gt_sizes) > 1):
        ap.error("a list of sizes needs --crop: full frames of different sizes cannot share a batch")
    recs = [dict(np.load(p)) for p in a.recordings]
    recs += [synthetic_recording(a.items, *sizes[k % len(sizes)], a.scale, a.window, a.sliding, a.seed + k, gt_sizes[k % len(gt_sizes)])
             for k in range(a.synthetic)]
    if a.save:
        os.makedirs(a.save, exist_ok=True)
        for k, r in enumerate(recs[len(a.recordings):]):
            np.savez(os.path.join(a.save, "synthetic%d.npz" % k), **r)
    mechanisms = (("Horizontal", "Vertical", "Polarity") if a.augment else ()) + (("Transpose",) if a.transpose is not None else ())
    probs = (0.5,) * (3 if a.augment else 0) + ((a.transpose,) if a.transpose is not None else ())
    ts = EventTrainSet(L=a.L, step_size=a.step_size, augment=(mechanisms, probs) if mechanisms else None,
                       pause=tuple(float(v) for v in a.pause.split(",")) if a.pause else None, add_noise=a.noise, window=a.window,
                       crop=crop, scale=a.scale)
    vs = None
    if a.valid_every > 0:
        if len(recs) < 2:
            raise SystemExit("--valid-every holds the last recording out: give at least two")
        vs = EventTrainSet(L=a.L, step_size=a.step_size, window=a.window)      # as recorded: no augmentation, pause or noise
        add(vs, recs.pop(), dev, a.window, a.sliding, a.scale, denoise, a.from_hr)
        if len(vs) < a.batch:
            raise SystemExit("the held-out recording gives %d sequences, fewer than one batch of %d" % (len(vs), a.batch))
    for r in recs:
        k = add(ts, r, dev, a.window, a.sliding, a.scale, denoise, a.from_hr)
        if denoise is not None:
            print("recording %d: noise filter dt %g support %d dropped %d of %d LR events" % ((k,) + denoise + (ts.noise_dropped(k), ts.synthesized_events(k) if a.from_hr is not None else len(r["lr_xs"]))))
    print("%d recordings, %d sequences of L = %d" % (len(recs), len(ts), a.L) + (", %dx%d patches" % crop if crop else "") +
          (", transposed with probability %g" % a.transpose if a.transpose is not None else "") +
          (", %d held-out sequences" % len(vs) if vs is not None else "") + (", loss %r" % loss_obj if loss_obj is not None else ""))
    random.seed(a.seed)
    torch.manual_seed(a.seed)
    m = BMCNet(a.scale, a.n_c, a.n_b).to(dev)
    if a.optimizer == "hip":
        from bmc_hip.optim import Adam
        opt = Adam(m.parameters(), lr=a.lr, max_grad_norm=a.clip_norm, nonfinite=a.nonfinite, ema_decay=a.ema, ema_warmup=a.ema_warmup)
    else:
        if a.nonfinite != "propagate":
            raise SystemExit("--nonfinite skip needs --optimizer hip (torch.optim.Adam cannot skip a step without a host sync)")
        opt = torch.optim.Adam(m.parameters(), lr=a.lr)
        if a.clip_norm is not None:
            clipped = list(m.parameters())
            opt.register_step_pre_hook(lambda *_: (torch.nn.utils.clip_grad_norm_(clipped, a.clip_norm), None)[1])
    g = torch.Generator().manual_seed(a.seed)
    rows, step, epoch, clock = [], 0, 0, None
    while step < a.steps:
        batches = ts.batches(a.batch, generator=g)
        if not batches:
            raise SystemExit("the recordings give %d sequences, fewer than one batch of %d" % (len(ts), a.batch))
        for idx in batches:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            inp, gt = ts.batch(idx)
            t1.record()
            loss, mse = bptt_step(m, opt, inp, gt, a.n_c, a.scale, **({"loss_fn": loss_obj} if loss_obj is not None else {}))
            loss = float(loss)
            rows.append(dict(step=step, epoch=epoch, sequences=idx, loss=loss, encode_ms=round(t0.elapsed_time(t1), 4)))
            if a.transpose is not None:
                rows[-1]["transposed"] = int((ts.last_flips & 8 != 0).sum())
            print("step %d  loss %.6f  encode %.3f ms  sequences %s" % (step, loss, rows[-1]["encode_ms"], idx))
            step += 1
            if vs is not None and step % a.valid_every == 0:
                validate = lambda: [float(valid_step(m, *vs.batch(vidx), a.n_c, a.scale, loss=loss_obj)[0])
                                    for vidx in vs.batches(a.batch, shuffle=False)]
                vl = validate()
                rows[-1]["valid_loss"] = sum(vl) / len(vl)
                if a.ema is not None:
                    with opt.ema_weights():                  # the same sequences on the averaged weights
                        ve = validate()
                    rows[-1]["valid_loss_ema"] = sum(ve) / len(ve)
                    print("step %d  valid_loss %.6f  valid_loss_ema %.6f  (%d batches)" % (
                        step - 1, rows[-1]["valid_loss"], rows[-1]["valid_loss_ema"], len(vl)))
                else:
                    print("step %d  valid_loss %.6f  (%d batches)" % (step - 1, rows[-1]["valid_loss"], len(vl)))
            if step == 1:
                torch.cuda.synchronize()
                clock = time.perf_counter()
            if step >= a.steps:
                break
        epoch += 1
    if a.wall and step > 1:
        torch.cuda.synchronize()
        print("optimizer %s: %.3f ms wall per step over steps 1..%d" % (a.optimizer, (time.perf_counter() - clock) * 1e3 / (step - 1), step - 1))
    if a.optimizer == "hip" and (a.clip_norm is not None or a.nonfinite == "skip"):
        norm, c = opt.last_clip().tolist()                   # once, at the end: the step itself never syncs
        print("last step: gradient norm %.6g, clip coefficient %.6g; %d of %d steps skipped" % (norm, c, int(opt.skipped_steps()), step))
    if a.save_ema:
        torch.save({k: v.detach().cpu() for k, v in opt.ema_state_dict(m).items()}, a.save_ema)
        print("EMA weights (decay %g%s) written to %s" % (a.ema, ", warm-up" if a.ema_warmup else "", a.save_ema))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f)


if __name__ == "__main__":
    main()
