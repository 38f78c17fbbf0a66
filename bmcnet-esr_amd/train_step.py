"""One BPTT training step with the semantics of the reference's hot loop (train.py:202-237):
zero_grad; for each sliding window: forward with the recurrent state carried WITHOUT detach, MSE against the HR
count image of the window's second frame, losses summed; one backward over all windows; one optimizer step.
Other losses than the reference's MSE: a bmc_hip.losses object (L1, Huber, Charbonnier) as loss_fn / loss keeps the fused head; an
SSIM or Mix object adds the structural term on the head's prediction with the library's own kernels (ops.ssim_loss).

Plus the synthetic NFS-shaped event generator used by bench.py / tests."""
import torch
import torch.nn.functional as F

from bmc_hip import losses, ops


def synthetic_events(B, seql, H, W, scale, n_lr, device, seed=3407):
    """Per sample and frame: n_lr LR events and scale^2*n_lr HR events, x~U{0..W-1}, y~U{0..H-1}, p=+-1.
    Returns dict of flat fp32 vectors + int64 frame offsets (frame order: b-major, then time)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = {}
    for tag, (h, w, n) in {"lr": (H, W, n_lr), "hr": (H * scale, W * scale, n_lr * scale * scale)}.items():
        nf = B * seql
        xs = torch.randint(0, w, (nf * n,), generator=g).to(torch.float32)
        ys = torch.randint(0, h, (nf * n,), generator=g).to(torch.float32)
        ps = (torch.randint(0, 2, (nf * n,), generator=g) * 2 - 1).to(torch.float32)
        off = torch.arange(nf + 1, dtype=torch.int64) * n
        out[tag] = tuple(t.to(device) for t in (xs, ys, ps, off))
    return out


def shard_sequences(inp_cnt, gt_cnt, rank, world):
    """Sequence-batch sharding: rank r of `world` owns sequences [r*B/world, (r+1)*B/world) of the global
    batch -- what DistributedSampler does for the reference's loader (dataloader/h5dataloader.py:191-201); every rank
    then runs the full BPTT on its own sequences and GradAllReducer averages the gradients."""
    B = inp_cnt.shape[0]
    if B % world:
        raise ValueError("global batch %d is not divisible by %d ranks" % (B, world))
    n = B // world
    return inp_cnt[rank * n:(rank + 1) * n], gt_cnt[rank * n:(rank + 1) * n]


def encode_sequence(ev, B, seql, H, W, scale):
    """events -> inp_cnt [B,seql,2,H,W], gt_cnt [B,seql,2,sH,sW] on the GPU (two batched scatter launches);
    what the reference's DataLoader workers do per frame with events_to_channels (dataloader/h5dataset.py:518-526)."""
    xs, ys, ps, off = ev["lr"]
    inp = ops.events_to_channels_batched(xs, ys, ps, off, H, W, mutate=False).view(B, seql, 2, H, W)
    xs, ys, ps, off = ev["hr"]
    gt = ops.events_to_channels_batched(xs, ys, ps, off, H * scale, W * scale, mutate=False).view(
        B, seql, 2, H * scale, W * scale)
    return inp, gt


def bptt_step(model, optimizer, inp_cnt, gt_cnt, n_c, scale, seqn=2, plain=False, loss_fn=F.mse_loss, recompute=False):
    """inp_cnt [B,L,2,H,W], gt_cnt [B,L,2,sH,sW] (device tensors).  Returns (loss, last mse).

    recompute=True keeps only the recurrent state (h, hp, hn, prediction) of every window and re-runs a window's
    forward inside backward (activation checkpointing per window): peak memory drops from
    windows x (one window's activations) to one window's activations, at the price of one extra forward per
    window.  Needed for long sequences / big batches (BASELINE configs[4]: T=16, 8 sequences per GPU); results
    are bit-identical (same kernels, same order).

    loss_fn: F.mse_loss (the reference's nn.MSELoss) and INSTANCES of bmc_hip.losses.L1 / Huber / Charbonnier are computed by
    the head kernel (model.forward_loss); INSTANCES of bmc_hip.losses.SSIM / Mix go through forward_loss too (the head, the
    resize where the sizes differ, ops.ssim_loss; a Mix keeps its pointwise term on the head kernel); every other callable --
    F.l1_loss, a lambda around one of those objects -- gets the unfused chain: model(), ops.bicubic_resize where the sizes
    differ, loss_fn and its autograd."""
    from torch.utils.checkpoint import checkpoint
    B, L, _, H, W = inp_cnt.shape
    dev = inp_cnt.device
    optimizer.zero_grad()
    loss = 0
    init = True
    z = lambda c: torch.zeros(B, c, H, W, device=dev)
    for i in range(L - seqn + 1):
        x = inp_cnt[:, i:i + seqn].transpose(1, 2)          # [B,2(pol),seqn,H,W]   (train.py:211)
        gt = gt_cnt[:, i + 1]                                # (train.py:213)
        # nn.MSELoss: head + loss in one kernel pass (models.*.forward_loss), whatever the ground truth's size -- another size
        # than the prediction's is the bicubic branch of train.py:227-231, resized inside that pass.  A bmc_hip.losses object:
        # the same pass with its rho (forward_loss(..., loss=loss_fn)).  Any other loss_fn object (a wrapper around F.mse_loss
        # or around a losses object included) selects the unfused chain below.
        robust = losses.on_device_path(loss_fn)
        fused = (loss_fn is F.mse_loss or robust) and hasattr(model, "forward_loss")
        fn = model.forward_loss if fused else model
        extra = (gt,) if fused else ()
        kw = {"loss": loss_fn} if fused and robust else {}
        if init:
            state = (z(n_c), z(2 * scale * scale)) if plain else (z(n_c), z(n_c), z(n_c), z(2 * scale * scale))
            out = fn(x, *state, True, *extra, **kw)
            init = False
        elif recompute:
            out = checkpoint(fn, x, *state, False, *extra, use_reentrant=False, **kw)
        else:
            out = fn(x, *state, False, *extra, **kw)
        if fused:
            state, mse = tuple(out[:-1]), out[-1]
        else:
            state = tuple(out)
            # size-mismatch branch of train.py:227-231 (EventZoom: 124x224 prediction vs 124x222 ground truth); the
            # UNRESIZED prediction is what recurs into the next window (train.py:224)
            mse = loss_fn(ops.bicubic_resize(state[-1], gt.shape[-2:]), gt)
        loss = loss + mse
    loss.backward()
    optimizer.step()
    return loss.detach(), mse.detach()


def valid_step(model, inp_cnt, gt_cnt, n_c, scale, seqn=2, plain=False, loss=None):
    """The body of the reference's _valid loop (train.py:479-509) for one batch: model.eval() under torch.no_grad(), the
    windows as in bptt_step with the state carried, the window losses (nn.MSELoss, against the bicubic-resized prediction
    where the ground truth has another size, train.py:502-506) summed through forward_loss.  No backward, no optimizer;
    nothing of the ground truth's size is allocated.  loss: None = nn.MSELoss; a bmc_hip.losses object (L1, Huber, Charbonnier)
    = that loss through the same fused head; an SSIM / Mix object = forward_loss with ops.ssim_loss, forward only (the resized
    prediction is allocated where the sizes differ); any other callable = the unfused chain (model(), ops.bicubic_resize where
    the sizes differ, the callable).  Returns (loss, last window's loss); the model's training mode is restored."""
    B, L, _, H, W = inp_cnt.shape
    dev = inp_cnt.device
    z = lambda c: torch.zeros(B, c, H, W, device=dev)
    loss_fn = None if loss is F.mse_loss else loss
    fused = loss_fn is None or losses.on_device_path(loss_fn)
    kw = {} if loss_fn is None else {"loss": loss_fn}
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            loss = 0
            state = (z(n_c), z(2 * scale * scale)) if plain else (z(n_c), z(n_c), z(n_c), z(2 * scale * scale))
            for i in range(L - seqn + 1):
                x = inp_cnt[:, i:i + seqn].transpose(1, 2)
                gt = gt_cnt[:, i + 1]
                if fused:
                    out = model.forward_loss(x, *state, i == 0, gt, **kw)
                    state, mse = tuple(out[:-1]), out[-1]
                else:
                    state = tuple(model(x, *state, i == 0))
                    mse = loss_fn(ops.bicubic_resize(state[-1], gt.shape[-2:]), gt)
                loss = loss + mse
    finally:
        model.train(was_training)
    return loss, mse
