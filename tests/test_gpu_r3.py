"""GPU parity tests added in round 3 (-m gpu), all through the C ABI of libbmc_hip.so: world-size-2 runs of the HIP path on
one GPU, the full-size C2 step, the inference row (SEQN = 3 inputs, bicubic baseline metric, non-aliased graph outputs)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
from test_gpu_r2 import _gpu, load, oracle_params, rel_l2, scaled_init, _restore_math_mode  # noqa: E402,F401
from parity_bars import *  # noqa: E402,F401,F403


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def _run_ranks(tmp_path, tag, world, backend, devices, accum, batch=4, side="auto"):
    port = _free_port()
    procs, outs = [], []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   BMC_ACCUM_GRADS=accum, HSA_ENABLE_IPC_MODE_LEGACY="0", BMC_RANK_TEST_B=str(batch), BMC_WGRAD_STREAM=side)
        out = str(tmp_path / ("%s_rank%d.npz" % (tag, r)))
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "rank_worker.py"), out, backend, str(devices[r])],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        logs.append(o)
    for p, o in zip(procs, logs):
        assert p.returncode == 0, o[-3000:]
    return [np.load(o) for o in outs]


def _full_batch_reference(dev):
    from rank_worker import problem
    from train_step import bptt_step
    m, inp, gt, n_c, scale = problem(dev)
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    loss, _ = bptt_step(m, opt, inp, gt, n_c, scale)
    return loss.item(), [(p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().numpy() for p in m.parameters()]


@pytest.mark.parametrize("accum,side", [("1", "auto"), ("0", "auto"), ("1", "1")])
def test_two_ranks_on_one_gpu_hip_step_matches_full_batch(tmp_path, accum, side):
    """world = 2 on the ONE GPU of the test box: two fresh processes on cuda:0, backend gloo (RCCL refuses two ranks on one
    device; the reducer moves its buckets through host memory for gloo), each running the real sharded step on the HIP
    kernels.  Everything of the N > 1 path except the RCCL transport: sequence sharding, kernel-side .grad accumulation
    (BMC_ACCUM_GRADS=1: no hook fires, finish() stages every bucket) or hook-driven buckets launched during backward
    (BMC_ACCUM_GRADS=0), averaging, .grad views.  == the single-process full batch to 1e-4; ranks bit-equal.
    side = "1": the weight-gradient kernels on the second stream (what large frames do by default; forced at this tiny size) --
    the reducer must see the gradients only after the streams have joined."""
    dev = _gpu()
    res = _run_ranks(tmp_path, "gloo%s%s" % (accum, side), 2, "gloo", [0, 0], accum, side=side)
    assert all(bool(r["side_stream"]) == (side == "1") for r in res)
    loss, grads = _full_batch_reference(dev)
    assert all(int(r["accum"]) == int(accum) for r in res)
    assert abs(0.5 * (float(res[0]["loss"]) + float(res[1]["loss"])) - loss) < 1e-5 * abs(loss)
    worst = 0.0
    for r in res:
        for i, g in enumerate(grads):
            worst = max(worst, rel_l2(r["g%03d" % i], g))
    print("2 ranks / 1 GPU, BMC_ACCUM_GRADS=%s: worst gradient rel-L2 vs full batch %.2e, buckets %d, launched from hooks %d"
          % (accum, worst, int(res[0]["nbuckets"]), int(res[0]["hook_launches"])))
    assert worst < 1e-4
    for i in range(len(grads)):
        assert np.array_equal(res[0]["g%03d" % i], res[1]["g%03d" % i])
    # the two routes really are different code paths: with kernel-side accumulation only the few parameters that reach
    # autograd (derived weights: conv_fs slices, stacked head weights) can complete a bucket during backward
    # (BMCNet(.., n_b=1): the only block is the last one, whose local BIE never evaluates v2 -- that parameter's bucket is
    # completed by finish() in either mode)
    if accum == "0":
        assert int(res[0]["hook_launches"]) >= max(1, int(res[0]["nbuckets"]) - 2)
    else:
        assert int(res[0]["hook_launches"]) <= 1


@pytest.mark.parametrize("world,accum", [(4, "1"), (4, "0"), (8, "1")])
def test_four_and_eight_ranks_on_one_gpu_hip_step_matches_full_batch(tmp_path, world, accum):
    """The same at world = 4 (both gradient routes) and world = 8 (the route the bench uses): 4 / 8 fresh processes on the one
    GPU, gloo transport, 8 sequences sharded 2 / 1 per rank -- the world sizes of the 1 / 2 / 4 / 8-GPU scaling runs, which no
    8-GPU node has been available to execute."""
    dev = _gpu()
    os.environ["BMC_RANK_TEST_B"] = "8"
    try:
        res = _run_ranks(tmp_path, "gloo%d_%s" % (world, accum), world, "gloo", [0] * world, accum, batch=8)
        loss, grads = _full_batch_reference(dev)
    finally:
        os.environ.pop("BMC_RANK_TEST_B", None)
    assert abs(sum(float(r["loss"]) for r in res) / world - loss) < 1e-5 * abs(loss)
    worst = max(rel_l2(r["g%03d" % i], g) for r in res for i, g in enumerate(grads))
    print("%d ranks / 1 GPU, BMC_ACCUM_GRADS=%s: worst gradient rel-L2 vs full batch %.2e, buckets %d, launched from hooks %d"
          % (world, accum, worst, int(res[0]["nbuckets"]), int(res[0]["hook_launches"])))
    assert worst < 1e-4
    for r in res[1:]:
        for i in range(len(grads)):
            assert np.array_equal(res[0]["g%03d" % i], r["g%03d" % i])


def test_two_ranks_rccl_hip_step_matches_full_batch(tmp_path):
    """The same over RCCL, one rank per GPU (needs two GPUs: skipped on the 1-GPU test box)."""
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    dev = _gpu()
    res = _run_ranks(tmp_path, "rccl", 2, "nccl", [0, 1], "1")
    loss, grads = _full_batch_reference(dev)
    for r in res:
        for i, g in enumerate(grads):
            assert rel_l2(r["g%03d" % i], g) < 1e-4
    for i in range(len(grads)):
        assert np.array_equal(res[0]["g%03d" % i], res[1]["g%03d" % i])


# ------------------------------------------------------------------ inference row (infer_BMCNet.py:44-86)
@pytest.mark.parametrize("graph", [False, True])
def test_inference_loop_seqn3_golden(graph):
    """The reference's inference loop body on its own model class (golden infer_seqn3.npz, make_golden_r3.py): SEQN = 3
    inputs [B,2,3,H,W] (infer_BMCNet.py:147), predictions, esr_mse with the size-mismatch branch, and the bicubic baseline
    metric -- through StreamingSR, eager and with HIP-graph replay; the returned predictions are the caller's (collected
    WITHOUT cloning and compared after the last window)."""
    dev = _gpu()
    from infer import StreamingSR
    from models.BMCNet import BMCNet
    from test_gpu_parity import _load_sd
    z = load("infer_seqn3.npz")
    scale, n_c, n_b, B, H, W, seqn, nwin, gh, gw = (int(v) for v in z["meta"])
    m = BMCNet(scale, n_c, n_b)
    _load_sd(m, z); m.to(dev)
    frames, gts = torch.tensor(z["frames"]).to(dev), torch.tensor(z["gts"]).to(dev)
    sr = StreamingSR(m, n_c=n_c, scale=scale, graph=graph)
    kept, esr, base = [], [], []
    for i in range(nwin):
        x = frames[:, i:i + seqn].transpose(1, 2)
        assert x.shape[2] == 3
        pred = sr.step(x)
        kept.append(pred)
        esr.append(StreamingSR.esr_mse(pred, gts[:, i + 1]).item())
        base.append(StreamingSR.bicubic_mse(frames[:, i:i + seqn][:, 1], gts[:, i + 1], (gh, gw)).item())
    for i in range(nwin):
        assert rel_l2(kept[i], z["pred%d" % i]) < 1e-4, (i, graph)
        assert abs(esr[i] - float(z["esr_mse%d" % i])) < 1e-4 * float(z["esr_mse%d" % i])
        assert abs(base[i] - float(z["bicubic_mse%d" % i])) < 1e-5 * float(z["bicubic_mse%d" % i])
    if graph:
        assert sr._graph is not None
        # frame 2 of a window is never read (models/BMCNet.py:106-107): a 2-frame input replays the same graph? no -- the
        # captured input buffer has 3 frames, a different shape must be refused, not broadcast
        with pytest.raises(RuntimeError, match="differs from the captured"):
            sr.step(frames[:, 0:2].transpose(1, 2))
        with pytest.raises(RuntimeError, match="does not match the carried state"):
            sr.step(frames[:1, 0:3].transpose(1, 2))


def test_streaming_graph_follows_weight_updates_and_reset():
    """A captured graph replays the packed weights it was captured with: load_state_dict / an optimizer-style in-place
    update must invalidate it (parameter version counters), reset() must drop the static state."""
    dev = _gpu()
    from infer import StreamingSR
    from models.BMCNet import BMCNet
    torch.manual_seed(5)
    scale, n_c, n_b, B, H, W = 4, 16, 1, 1, 10, 16
    m = BMCNet(scale, n_c, n_b).to(dev)
    scaled_init(m, 4.0)
    g = torch.Generator().manual_seed(3)
    frames = torch.poisson(torch.full((B, 8, 2, H, W), 0.5), generator=g).to(dev)
    win = lambda i: frames[:, i:i + 2].transpose(1, 2)
    sr = StreamingSR(m, n_c=n_c, scale=scale, graph=True)
    for i in range(4):
        sr.step(win(i))
    assert sr._graph is not None
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.1)                                 # an "optimizer step"
    ref = StreamingSR(m, n_c=n_c, scale=scale, graph=False)
    ref.state = tuple(t.clone() for t in sr.state)
    ref._calls = sr._calls
    a, b = sr.step(win(4)), ref.step(win(4))
    assert torch.equal(a, b)                            # re-captured with the new weights (same kernels, same order)
    a, b = sr.step(win(5)), ref.step(win(5))
    assert torch.equal(a, b)
    sr.reset()
    assert sr._graph is None and sr._state_static is None and sr.state is None
    first = sr.step(win(0))
    ref.reset()
    assert torch.equal(first, ref.step(win(0)))


# ------------------------------------------------------------------ BASELINE configs[1] (C2) at its full size
def test_c2_full_size_window_forward_backward_vs_oracle():
    """One BMCNet(4,128,5) window at the C2 frame size (180x240 -> 720x960), B = 1, forward AND backward against the CPU
    oracle's autograd (round 2 checked C2's backward at a quarter frame only): loss <= 1e-5, every parameter gradient
    <= 1e-3 (measured ~1e-5).  Includes the conv_fs partial-column launches and the grouped conv_hp / conv_hn launch at
    full size.  ~10 s of CPU."""
    dev = _gpu()
    from models.BMCNet import BMCNet
    from oracle import bmc_oracle as O
    scale, n_c, n_b, B, H, W = 4, 128, 5, 1, 180, 240
    torch.manual_seed(71)
    m = BMCNet(scale, n_c, n_b)
    scaled_init(m, 2.0)
    params = oracle_params(m)
    g = torch.Generator().manual_seed(72)
    frames = torch.poisson(torch.full((B, 3, 2, H, W), 0.284), generator=g)
    gts = torch.poisson(torch.full((B, 3, 2, scale * H, scale * W), 0.284), generator=g)
    xs = [frames[:, i:i + 2].transpose(1, 2) for i in range(2)]
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    # two windows, so that the recurrent inputs (states, unshuffled previous prediction) carry gradient too
    loss_ref, preds_ref, _ = O.bptt_loss(params, xs, [gts[:, 1], gts[:, 2]], n_c, scale)
    loss_ref.backward()
    m.to(dev)
    z = lambda c: torch.zeros(B, c, H, W, device=dev)
    st = (z(n_c), z(n_c), z(n_c), z(2 * scale * scale))
    loss = 0
    for i in range(2):
        st = m(xs[i].to(dev), *st, i == 0)
        within(rel_l2(st[-1], preds_ref[i]), BAR_C2_SR, CONTRACT_SR, "C2 full size, SR of window %d" % i)
        loss = loss + F.mse_loss(st[-1], gts[:, i + 1].to(dev))
    loss.backward()
    within(abs(loss.item() - loss_ref.item()) / abs(loss_ref.item()), 2e-6, 1e-5, "C2 full size, loss")
    errs = {n: rel_l2(p.grad, params[n].grad) for n, p in m.named_parameters() if params[n].grad is not None}
    assert len(errs) >= 50
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
    print("C2 full-size 2-window fwd+bwd: loss %.6f vs %.6f, worst gradients %s" % (loss.item(), loss_ref.item(), [(n, "%.1e" % e) for n, e in worst]))
    within(worst[0][1], BAR_C2_GRAD, CONTRACT_GRAD, "C2 full size, worst parameter gradient (%s)" % worst[0][0])


def test_c2_full_step_batch4_8_windows_properties():
    """The bench's own step at its full size (BASELINE configs[1]: bs 4, SEQL 9 -> 8 windows, 180x240, store-everything:
    ~140 GiB) through size-independent properties: the step's gradient is the mean of its two half-batches' gradients and
    its loss the mean of theirs (MSE is a batch mean, sequences are independent: what batch sharding relies on), and a
    slice of it is bit-identical with per-window recompute."""
    dev = _gpu()
    from models.BMCNet import BMCNet
    from train_step import bptt_step
    scale, n_c, n_b, B, L, H, W = 4, 128, 5, 4, 9, 180, 240
    torch.manual_seed(73)
    m = BMCNet(scale, n_c, n_b).to(dev)
    scaled_init(m, 2.0)
    g = torch.Generator().manual_seed(74)
    inp = torch.poisson(torch.full((B, L, 2, H, W), 0.284), generator=g).to(dev)
    gt = torch.poisson(torch.full((B, L, 2, scale * H, scale * W), 0.284), generator=g).to(dev)
    opt = torch.optim.SGD(m.parameters(), lr=0.0)

    def step(sl, recompute=False, nwin=L):
        torch.cuda.reset_peak_memory_stats()
        loss, _ = bptt_step(m, opt, inp[sl, :nwin], gt[sl, :nwin], n_c, scale, recompute=recompute)
        grads = [p.grad.clone() for p in m.parameters()]
        return loss.item(), grads, torch.cuda.max_memory_allocated() / 2 ** 30

    l_all, g_all, mem = step(slice(0, 4))
    print("C2 full step: loss %.6f peak %.1f GiB" % (l_all, mem))
    assert np.isfinite(l_all) and mem < 220.0
    l_a, g_a, _ = step(slice(0, 2))
    l_b, g_b, _ = step(slice(2, 4))
    assert abs(l_all - 0.5 * (l_a + l_b)) < 2e-6 * abs(l_all)
    worst = max(rel_l2(ga, 0.5 * (a + b)) for ga, a, b in zip(g_all, g_a, g_b))
    assert worst < 2e-4, worst
    l_r, g_r, _ = step(slice(0, 2), True, 4)
    l_s, g_s, _ = step(slice(0, 2), False, 4)
    assert l_r == l_s and all(torch.equal(a, b) for a, b in zip(g_r, g_s))


# ------------------------------------------------------------------ event encoders: LDS-binned path, long voxel segments
def test_binned_event_scatter_bit_exact_vs_oracle_and_atomic_kernel():
    """bmc_events_to_channels_binned (counting sort by row band + LDS count images, csrc/scatter.hip) on HR-sized frames
    with ragged / empty frames, out-of-range events of both polarities, float coordinates and a hot pixel: identical bit
    for bit to the numpy oracle and to the atomic kernel, including the in-place reset of out-of-range coordinates."""
    dev = _gpu()
    from bmc_hip import ops
    from oracle import bmc_oracle as O
    H, W = 720, 960
    rng = np.random.default_rng(5)
    counts = [393216, 0, 1000, 200001, 7]
    xs, ys, ps = [], [], []
    for n in counts:
        x = rng.uniform(-3.0, W + 3.0, n).astype(np.float32)
        y = rng.uniform(-3.0, H + 3.0, n).astype(np.float32)
        if n > 5000:
            x[:3000], y[:3000] = 17.5, 700.25            # a hot pixel
            x[3000:3400], y[3000:3400] = -1.0, 5.0       # out of range, both polarities
        xs.append(x); ys.append(y); ps.append(rng.choice([-1.0, 1.0], n).astype(np.float32))
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device=dev)
    cat = lambda l: torch.tensor(np.concatenate(l), device=dev)
    assert H * W >= ops.BINNED_MIN_PIXELS
    x1, y1, p1 = cat(xs), cat(ys), cat(ps)
    got = ops.events_to_channels_batched(x1, y1, p1, off, H, W, mutate=True)
    old = ops.BINNED_MIN_PIXELS
    try:
        ops.BINNED_MIN_PIXELS = 1 << 40                      # force the atomic kernel
        x2, y2, p2 = cat(xs), cat(ys), cat(ps)
        ref_gpu = ops.events_to_channels_batched(x2, y2, p2, off, H, W, mutate=True)
    finally:
        ops.BINNED_MIN_PIXELS = old
    assert torch.equal(got, ref_gpu) and torch.equal(x1, x2) and torch.equal(y1, y2)
    for f, n in enumerate(counts):
        img, xa, ya = O.events_to_channels_np(xs[f], ys[f], ps[f], (H, W))
        assert np.array_equal(got[f].cpu().numpy(), img), f
        a, b = int(off[f]), int(off[f + 1])
        assert np.array_equal(x1[a:b].cpu().numpy(), xa) and np.array_equal(y1[a:b].cpu().numpy(), ya)
    assert float(got.sum()) == float(sum(O.events_to_channels_np(xs[f], ys[f], ps[f], (H, W))[0].sum() for f in range(len(counts))))
    # mutate=False leaves the caller's arrays alone
    x3, y3 = cat(xs), cat(ys)
    ops.events_to_channels_batched(x3, y3, cat(ps), off, H, W, mutate=False)
    assert torch.equal(x3, cat(xs)) and torch.equal(y3, cat(ys))


def test_binned_raw_column_encoder_bit_exact_at_hr_size():
    dev = _gpu()
    from bmc_hip import ops
    from oracle import bmc_oracle as O
    H, W = 720, 960
    rng = np.random.default_rng(6)
    counts = [150000, 393216, 3]
    flags = [5, 2, 7]
    xs = [rng.integers(-2, W + 2, n).astype(np.int16) for n in counts]
    ys = [rng.integers(-2, H + 2, n).astype(np.int16) for n in counts]
    ps = [rng.choice([-1.0, 1.0], n).astype(np.float64) for n in counts]
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device=dev)
    got = ops.encode_raw_events(torch.tensor(np.concatenate(xs), device=dev), torch.tensor(np.concatenate(ys), device=dev),
                                torch.tensor(np.concatenate(ps), device=dev), off,
                                torch.tensor(flags, dtype=torch.uint8, device=dev), H, W)
    for f in range(len(counts)):
        assert np.array_equal(got[f].cpu().numpy(), O.encode_raw_frame_np(xs[f], ys[f], ps[f], flags[f], (H, W))), f


def test_voxel_long_segments_are_sorted_cooperatively():
    """every out-of-range event of a frame lands in ONE pixel's segment, hot pixels give long segments too, and
    the per-pixel pass sorted them with a single-thread insertion sort (O(k^2)).  50 000 + 20 000 such events now go
    through the workgroup-wide sort first: bit-exact vs the numpy oracle (event-order summation), in well under a second."""
    import time
    dev = _gpu()
    from bmc_hip import ops
    from oracle import bmc_oracle as O
    H, W, bins, n = 45, 80, 5, 90000
    rng = np.random.default_rng(8)
    xs = rng.uniform(0, W, n).astype(np.float32)
    ys = rng.uniform(0, H, n).astype(np.float32)
    sel = rng.permutation(n)
    xs[sel[:50000]], ys[sel[:50000]] = -2.0, 3.0          # out of range -> pixel (H-1, 0) from the second bin on
    xs[sel[50000:70000]], ys[sel[50000:70000]] = 40.5, 20.5
    ts = np.sort(rng.uniform(0, 1, n)).astype(np.float32)
    ps = rng.choice([-1.0, 1.0], n).astype(np.float32)
    ref, xa, ya = O.events_to_voxel_np(xs, ys, ts, ps, bins, (H, W))
    d = [torch.tensor(a, device=dev) for a in (xs, ys, ts, ps)]
    off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    ops.events_to_voxel_batched(d[0].clone(), d[1].clone(), d[2], d[3], off, bins, H, W)      # warm-up (module load)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = ops.events_to_voxel_batched(d[0], d[1], d[2], d[3], off, bins, H, W)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("voxel with 50k + 20k event segments: %.1f ms" % (dt * 1e3))
    assert np.array_equal(got[0].cpu().numpy(), ref)
    assert np.array_equal(d[0].cpu().numpy(), xa) and np.array_equal(d[1].cpu().numpy(), ya)
    assert dt < 0.5


# One scan launch (csrc/scatter.hip::table_scan_kernel, 1 024 threads a table) serves the binned encoder, the voxel frames and the
# torch-tensor image: tables of one entry, of one entry more or less than its threads, and of several entries per thread.
@pytest.mark.parametrize("nframes", [1, 1023, 1024, 1025, 3000])
def test_scan_lengths_binned_encoder(nframes):
    """3 x 5 frames are one row band each, so the (frame, band) table has nframes entries; some frames are empty."""
    dev = _gpu()
    from bmc_hip import ops
    from oracle import bmc_oracle as O
    H, W = 3, 5
    rng = np.random.default_rng(nframes)
    counts = rng.integers(0, 7, nframes)
    counts[0] = 6
    n = int(counts.sum())
    xs = rng.uniform(-1.0, W + 1.0, n).astype(np.float32)
    ys = rng.uniform(-1.0, H + 1.0, n).astype(np.float32)
    ps = rng.choice([-1.0, 1.0], n).astype(np.float32)
    bounds = np.concatenate([[0], np.cumsum(counts)])
    off = torch.tensor(bounds, dtype=torch.int64, device=dev)
    old = ops.BINNED_MIN_PIXELS
    try:
        ops.BINNED_MIN_PIXELS = 0                            # force the binned path
        assert ops._binned_ws(n, nframes, H, W, dev) is not None
        got = ops.events_to_channels_batched(*(torch.tensor(a, device=dev) for a in (xs, ys, ps)), off, H, W, mutate=False)
    finally:
        ops.BINNED_MIN_PIXELS = old
    got = got.cpu().numpy()
    for f in range(nframes):
        a, b = bounds[f], bounds[f + 1]
        assert np.array_equal(got[f], O.events_to_channels_np(xs[a:b], ys[a:b], ps[a:b], (H, W))[0]), f


@pytest.mark.parametrize("H,W", [(1, 1), (33, 31), (32, 32), (25, 41), (45, 80)])
def test_scan_lengths_voxel_frames_and_torch_image(H, W):
    """Tables of 1, 1 023, 1 024, 1 025 and 3 600 pixels: three voxel frames (one table each, the middle frame empty) and the
    single table of events_to_image_torch, against the numpy oracle, bit for bit."""
    dev = _gpu()
    from bmc_hip import encodings as E, ops
    from oracle import bmc_oracle as O
    rng = np.random.default_rng(H * 100 + W)
    bins, m = 5, 2 * H * W + 9
    counts = [m, 0, m + 3]
    n = sum(counts)
    xs = np.floor(rng.uniform(-0.2, W + 0.2, n)).astype(np.float32)
    ys = np.floor(rng.uniform(-0.2, H + 0.2, n)).astype(np.float32)
    ts = np.concatenate([np.sort(rng.uniform(0, 1, c)) for c in counts]).astype(np.float32)
    ps = rng.choice([-1.0, 1.0], n).astype(np.float32)        # polarities; float weights and other bin counts: test_gpu_voxel_bins.py
    bounds = np.concatenate([[0], np.cumsum(counts)])
    d = [torch.tensor(a, device=dev) for a in (xs, ys, ts, ps)]
    got = ops.events_to_voxel_batched(d[0], d[1], d[2], d[3], torch.tensor(bounds, dtype=torch.int64, device=dev), bins, H, W)
    for f in range(len(counts)):
        a, b = bounds[f], bounds[f + 1]
        ref, xa, ya = O.events_to_voxel_np(xs[a:b], ys[a:b], ts[a:b], ps[a:b], bins, (H, W))
        assert np.array_equal(got[f].cpu().numpy(), ref), f
        assert np.array_equal(d[0][a:b].cpu().numpy(), xa) and np.array_equal(d[1][a:b].cpu().numpy(), ya), f
    pw = rng.standard_normal(n).astype(np.float32)            # the image adds arbitrary weights in event order
    ref = O.events_to_image_torch_np(xs.copy(), ys.copy(), pw.copy(), (H, W))
    img = E.events_to_image_torch(*(torch.tensor(a.copy(), device=dev) for a in (xs, ys, pw)), sensor_size=(H, W))
    assert np.array_equal(img.cpu().numpy(), ref)


# ------------------------------------------------------------------ Winograd F(2x2, 3x3) convolution kernel (csrc/wino.hip)
@pytest.fixture(params=[8, 4], ids=["rows8", "rows4"])
def force_wino(request, monkeypatch):
    """Send every eligible 3x3 launch through the Winograd kernel, whatever its size (default: only launches that fill the chip),
    once with each of its two workgroup tilings (8 x 16 and 4 x 16 pixels: csrc/wino.hip::wino_rows picks by launch size)."""
    from bmc_hip import ops
    old = ops.WINO_MIN_TILES
    ops.WINO_MIN_TILES = 0
    monkeypatch.setenv("BMC_WINO_TH", str(request.param))
    ops._WINO_ROWS.clear()
    yield ops
    ops.WINO_MIN_TILES = old
    monkeypatch.delenv("BMC_WINO_TH")
    ops._WINO_ROWS.clear()


@pytest.mark.parametrize("B,H,W,cins,cout,relu,res", [
    (1, 8, 16, [128], 128, True, False),              # exactly one tile
    (2, 9, 7, [128], 128, False, False),              # ragged in both directions, partial tiles only
    (2, 19, 37, [128], 128, True, True),
    (2, 13, 21, [16, 128, 16], 128, True, False),     # multi-source: narrow sources' data gradients stay on the direct kernel
    (1, 11, 18, [16, 128, 16, 16, 32], 128, True, False),
    (2, 5, 40, [256], 256, False, True),              # two channel tiles, 16 chunks
    (3, 17, 33, [32], 128, False, False),
])
def test_winograd_conv_fwd_bwd_vs_float64(force_wino, B, H, W, cins, cout, relu, res):
    dev = _gpu()
    ops = force_wino
    from bmc_hip.ops import ConvSpec, View
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W)
    xs = [torch.randn(B, c, H, W, generator=g) for c in cins]
    cin = sum(cins)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    b = torch.randn(cout, generator=g)
    r = torch.randn(B, cout, H, W, generator=g) if res else None
    go = torch.randn(B, cout, H, W, generator=g)
    xs_c = [x.double().requires_grad_() for x in xs]
    w_c, b_c = w.double().requires_grad_(), b.double().requires_grad_()
    r_c = r.double().requires_grad_() if res else None
    y = F.conv2d(torch.cat(xs_c, 1), w_c, b_c, padding=1)
    if res:
        y = y + r_c
    if relu:
        y = torch.relu(y)
    y.backward(go.double())
    assert ops.wino_ok(B, H, W, cout, 9)
    xs_g = [nhwc(x).to(dev).requires_grad_() for x in xs]
    w_g, b_g = w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    r_g = nhwc(r).to(dev).requires_grad_() if res else None
    ops.PROFILE, ops.PROFILE_WINO[:] = [], [0, 0]
    yg = ops.conv([View(x) for x in xs_g], w_g, b_g, ConvSpec.dense(*cins), relu=relu, residual=View(r_g) if res else None)
    yg.backward(nhwc(go).to(dev))
    ops.PROFILE = None
    assert ops.PROFILE_WINO[0] >= 1 + sum(1 for c in cins if c % 128 == 0), ops.PROFILE_WINO      # the kernel under test really ran
    assert rel_l2(yg.permute(0, 3, 1, 2), y) < 3e-6
    for xg, xc in zip(xs_g, xs_c):
        assert rel_l2(xg.grad.permute(0, 3, 1, 2), xc.grad) < 3e-6
    assert rel_l2(w_g.grad, w_c.grad) < 2e-5
    assert rel_l2(b_g.grad, b_c.grad) < 2e-5
    if res:
        assert rel_l2(r_g.grad.permute(0, 3, 1, 2), r_c.grad) < 2e-5


def test_winograd_matches_direct_kernel_with_every_epilogue(force_wino):
    """The same launches through the direct fp32 kernel and through the Winograd kernel: bias in / out of the accumulators
    (per-group bias), residual with a batch rotation, ReLU, ReLU mask, accumulate, per-group weights, output written into a
    channel window of a wider tensor -- each within fp32 rounding of the other."""
    dev = _gpu()
    ops = force_wino
    from bmc_hip.ops import _packed_weight, _src, conv_raw, coutpad, ConvSpec
    torch.manual_seed(12)
    B, H, W, Cn = 4, 21, 35, 128
    spec = ConvSpec.dense(Cn)
    x = torch.randn(B, H, W, Cn, device=dev)
    res = torch.randn(B, H, W, Cn, device=dev)
    msk = torch.randn(B, H, W, Cn, device=dev)
    w = torch.randn(2, Cn, Cn, 9, device=dev) * 0.03
    bias = torch.randn(2, Cn, device=dev)
    cp = coutpad(Cn)

    def run(wino, G, relu, use_res, use_mask, accumulate, wide):
        w4 = w[:G].contiguous()
        wp = _packed_weight(w4, spec, None, wino=wino)
        Co = 2 * Cn if wide else Cn
        out = torch.full((B, H, W, Co), 0.25, device=dev)
        conv_raw([_src(x, 0, Cn, 0, None, 0, B)], wp, spec.kpad * 9 * cp, bias[:G].contiguous(), Cn,
                 out.data_ptr() + (4 * Cn if wide else 0), H * W * Co, Co, B, H, W, Cn, 9, relu=relu,
                 residual=_src(res, 0, Cn, 2, B, 0, B) if use_res else None, bpg=B // G, accumulate=accumulate,
                 mask=_src(msk, 0, Cn, 0, None, 0, B) if use_mask else None, wino=wino)
        return out

    for G, relu, use_res, use_mask, accumulate, wide in [(1, False, False, False, False, False), (1, True, True, False, False, False),
                                                         (2, False, False, True, False, False), (2, True, True, False, True, True),
                                                         (1, False, True, True, True, False)]:
        a, b = run(True, G, relu, use_res, use_mask, accumulate, wide), run(False, G, relu, use_res, use_mask, accumulate, wide)
        assert rel_l2(a, b) < 2e-6, (G, relu, use_res, use_mask, accumulate, wide)
        if wide:
            assert torch.equal(a[..., :Cn], torch.full_like(a[..., :Cn], 0.25))      # the other channel window is untouched


@pytest.mark.parametrize("tag", ["bmcnet_nc16", "bmcnet_nc32"])
def test_full_model_golden_unaffected_by_winograd_switch(force_wino, tag):
    """n_c = 16 / 32 models have no 128-channel convolution: the switch must not change a thing (eligibility is by shape)."""
    dev = _gpu()
    ops = force_wino
    assert not ops.wino_ok(4, 64, 64, 32, 9) and not ops.wino_ok(4, 64, 64, 16, 9)


def test_winograd_residual_blocks_and_bie_at_nc128_vs_oracle(force_wino):
    """BMCNet(4,128,1) on a small frame, two recurrent windows forward + backward with every 128-channel 3x3 launch (residual
    blocks, input-fusion and head convolutions, their data gradients) on the Winograd kernel, against the CPU oracle."""
    dev = _gpu()
    ops = force_wino
    from models.BMCNet import BMCNet
    from oracle import bmc_oracle as O
    scale, n_c, n_b, B, H, W = 4, 128, 1, 2, 20, 27
    torch.manual_seed(81)
    m = BMCNet(scale, n_c, n_b)
    scaled_init(m, 2.5)
    params = oracle_params(m)
    g = torch.Generator().manual_seed(82)
    frames = torch.poisson(torch.full((B, 3, 2, H, W), 0.4), generator=g)
    gts = torch.poisson(torch.full((B, 3, 2, scale * H, scale * W), 0.4), generator=g)
    xs = [frames[:, i:i + 2].transpose(1, 2) for i in range(2)]
    loss_ref, preds_ref, _ = O.bptt_loss(params, xs, [gts[:, 1], gts[:, 2]], n_c, scale)
    loss_ref.backward()
    m.to(dev)
    z = lambda c: torch.zeros(B, c, H, W, device=dev)
    st = (z(n_c), z(n_c), z(n_c), z(2 * scale * scale))
    loss = 0
    ops.PROFILE, ops.PROFILE_WINO[:] = [], [0, 0]
    for i in range(2):
        st = m(xs[i].to(dev), *st, i == 0)
        within(rel_l2(st[-1], preds_ref[i]), BAR_W128_SR, CONTRACT_SR, "BMCNet(4,128,1) 20x27, SR of window %d" % i)
        loss = loss + F.mse_loss(st[-1], gts[:, i + 1].to(dev))
    loss.backward()
    ops.PROFILE = None
    assert ops.PROFILE_WINO[0] > 40, ops.PROFILE_WINO
    within(abs(loss.item() - loss_ref.item()) / abs(loss_ref.item()), 2e-6, 1e-5, "loss")
    errs = {n: rel_l2(p.grad, params[n].grad) for n, p in m.named_parameters() if params[n].grad is not None}
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
    print("winograd BMCNet(4,128,1) 2 windows: %d winograd / %d direct conv launches, worst gradients %s" %
          (ops.PROFILE_WINO[0], ops.PROFILE_WINO[1], [(n, "%.1e" % e) for n, e in worst]))
    within(worst[0][1], BAR_W128_GRAD, CONTRACT_GRAD, "worst parameter gradient (%s)" % worst[0][0])


# ------------------------------------------------------------------ weight gradients on a side stream (small frames)
@pytest.mark.parametrize("math", ["fp32", "bf16"])
def test_side_stream_weight_gradients_are_bit_identical(math):
    """Small problems run their weight-gradient GEMMs + slab reductions on a side stream beside the data-gradient chain
    (bmc_hip.ops.wgrad_side).  Same kernels, same accumulation order per parameter: the whole step -- loss and every
    parameter gradient, three steps of Adam -- must be bit-identical to the single-stream run, in repeated runs."""
    dev = _gpu()
    from bmc_hip import ops
    from models.BMCNet import BMCNet
    from train_step import bptt_step
    ops.set_math(math)
    scale, n_c, n_b, B, L, H, W = 4, 128, 2, 2, 4, 31, 56
    g = torch.Generator().manual_seed(91)
    inp = torch.poisson(torch.full((B, L, 2, H, W), 0.5), generator=g).to(dev)
    gt = torch.poisson(torch.full((B, L, 2, scale * H, scale * W), 0.5), generator=g).to(dev)

    def run(mode):
        old = ops.WGRAD_SIDE
        ops.WGRAD_SIDE = mode
        try:
            torch.manual_seed(92)
            m = BMCNet(scale, n_c, n_b).to(dev)
            scaled_init(m, 2.0)
            opt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=1e-5, amsgrad=True)
            losses = []
            for _ in range(3):
                loss, _ = bptt_step(m, opt, inp, gt, n_c, scale)
                losses.append(loss.item())
            torch.cuda.synchronize()
            return losses, [p.grad.clone() for p in m.parameters() if p.grad is not None], [p.detach().clone() for p in m.parameters()]
        finally:
            ops.WGRAD_SIDE = old

    l0, g0, p0 = run("0")
    for rep in range(2):
        l1, g1, p1 = run("1")
        assert l0 == l1
        assert len(g0) == len(g1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
        assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    la, ga, pa = run("auto")         # (31x56: the automatic choice is one stream since round 4)
    assert la == l0 and all(torch.equal(a, b) for a, b in zip(ga, g0))
    assert ops._SIDE and not next(iter(ops._SIDE.values())).armed and not next(iter(ops._SIDE.values())).keep


# ------------------------------------------------------------------ Winograd weight-gradient kernel (csrc/wino_wgrad.hip)
def _wgrad_reference(x, g):
    """float64 weight / bias gradient of a 3x3 'same' convolution: x, g NHWC fp32 tensors -> (dW [Co,Ci,3,3], db [Co])."""
    import torch.nn.functional as F
    x64 = x.detach().cpu().double().permute(0, 3, 1, 2)
    g64 = g.detach().cpu().double().permute(0, 3, 1, 2)
    w = torch.zeros(g.shape[3], x.shape[3], 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(x64, w, padding=1) * g64).sum().backward()
    return w.grad, g64.sum((0, 2, 3))


@pytest.mark.parametrize("B,H,W", [
    (1, 2, 2),            # one tile, every neighbour outside the image
    (2, 7, 9),            # odd sizes: the last tile row / column are half outside
    (3, 4, 16),           # exactly one stage per image
    (2, 31, 56),          # configs[3] frame
    (5, 45, 80),          # the reference's own NFS frame; more stages than one workgroup per position row takes
    (1, 64, 100),
])
def test_winograd_weight_gradient_vs_float64(B, H, W):
    from bmc_hip import ops
    torch.manual_seed(B * 1000 + H * 10 + W)
    dev = torch.device("cuda:0")
    x = torch.randn(B, H, W, 128, device=dev)
    g = torch.randn(B, H, W, 128, device=dev)
    spec = ops.ConvSpec.dense(128)
    w = torch.zeros(128, 128, 3, 3, device=dev)
    b = torch.zeros(128, device=dev)
    assert ops.wino_wgrad_ok(ops._src(g, 0, 128, 0, None, 0, B), [ops._src(x, 0, 128, 0, None, 0, B)], spec, 9, 128, 1)
    dw, db = ops._wgrad_plain(g, x, spec, w, b, 9)
    ref_w, ref_b = _wgrad_reference(x, g)
    old = ops.WINO_WGRAD
    ops.WINO_WGRAD = False
    try:
        dw_d, db_d = ops._wgrad_plain(g, x, spec, w, b, 9)      # the pixel-reduction GEMM on the same operands
    finally:
        ops.WINO_WGRAD = old
    rel = lambda a, r: float((a.detach().cpu().double() - r).norm() / r.norm())
    e_w, e_b, e_d = rel(dw, ref_w), rel(db, ref_b), rel(dw_d, ref_w)
    print("B%d %dx%d: winograd dW %.2e db %.2e, direct dW %.2e" % (B, H, W, e_w, e_b, e_d))
    assert e_w < 2e-6 and e_b < 2e-6
    assert e_w < 4 * e_d + 1e-7          # fp32 Winograd: a small factor over the direct fp32 kernel's own rounding error
    # deterministic: a second launch gives the same bits
    dw2, db2 = ops._wgrad_plain(g, x, spec, w, b, 9)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def test_winograd_weight_gradient_views_accumulation_and_partial_columns():
    """The launch forms the model uses: operands that are batch windows of larger tensors, gradients accumulated straight into
    a leaf parameter's .grad (sink route, twice), and a launch that owns columns [256, 384) of a wider weight (conv_fs)."""
    from bmc_hip import ops
    torch.manual_seed(5)
    dev = torch.device("cuda:0")
    B, H, W = 2, 11, 18
    xbig = torch.randn(3 * B, H, W, 128, device=dev)
    g = torch.randn(B, H, W, 128, device=dev)
    x = xbig[B:2 * B]
    ref_w, ref_b = _wgrad_reference(x, g)
    spec = ops.ConvSpec.dense(128)
    w = torch.nn.Parameter(torch.zeros(128, 128, 3, 3, device=dev))
    b = torch.nn.Parameter(torch.zeros(128, device=dev))
    ops.set_accumulate_param_grads(True)
    for _ in range(2):
        dw, db = ops._wgrad_plain(g, x, spec, w, b, 9)
        assert dw is None and db is None
    rel = lambda a, r: float((a.detach().cpu().double() - r).norm() / r.norm())
    assert rel(w.grad, 2 * ref_w) < 2e-6 and rel(b.grad, 2 * ref_b) < 2e-6
    # partial columns of a 288-input-channel weight through the generic convolution node
    wide = torch.nn.Parameter(torch.randn(128, 288, 3, 3, device=dev) * 0.05)
    sp = ops.ConvSpec([list(range(144, 272))], cin=288)
    xin = x.clone().requires_grad_(True)
    y = ops.conv([ops.View(xin)], wide, None, sp)
    (y * g).sum().backward()
    got = wide.grad.detach().cpu().double()
    assert rel(got[:, 144:272], ref_w) < 2e-6
    assert float(got[:, :144].abs().max()) == 0 and float(got[:, 272:].abs().max()) == 0


# ------------------------------------------------------------------ conv1p.hip: 1x1 convolution with register-resident weights
def test_conv1p_kernel_all_epilogues_vs_float64_and_old_kernels():
    """Child processes with BMC_CONV1P_MIN_TILES=0 (every eligible 1x1 problem takes conv1p.hip, whatever its size) and with
    BMC_CONV1P=0 (conv1.hip / conv.hip as before): K = 128 / 256 from one to three sources, 128 / 256 output channels, batch
    maps, per-sample weights, bias, residual with rotation, ReLU, mask, accumulate, ragged images (partial last tile)."""
    import json, os, subprocess, sys
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import os, sys, json
import torch
sys.path[:0] = [ROOT, os.path.join(ROOT, "bmcnet-esr_amd")]
from bmc_hip import ops
from bmc_hip.ops import ConvSpec, _src, conv_raw, _packed_weight, coutpad
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(11)
out = []
srcsets = [[128], [64, 64], [128, 128], [16, 112], [32, 96, 128], [256], [128], [128, 128]]
for case in range(16):
    B = int(torch.randint(1, 5, (1,), generator=g)); H = int(torch.randint(3, 40, (1,), generator=g)); W = int(torch.randint(3, 50, (1,), generator=g))
    nchs = srcsets[case % 8]
    Cout = [128, 128, 256, 100][case % 4]
    G = [1, B, 1, 1][case % 4] if B > 1 else 1
    relu, use_res, use_mask, acc, bias = case % 2 == 0, case % 3 == 0, case % 5 == 1, case % 4 == 2, case % 3 != 1
    xs = [torch.randn(B, H, W, c, generator=g).to(dev) for c in nchs]
    cin = sum(nchs)
    w = (torch.randn(G, Cout, cin, 1, generator=g) / cin ** 0.5).to(dev)
    b = (torch.randn(G, Cout, generator=g) * 0.3).to(dev) if bias else None
    res = torch.randn(B, H, W, Cout, generator=g).to(dev) if use_res else None
    mask = torch.randn(B, H, W, Cout, generator=g).to(dev) if use_mask else None
    base = torch.randn(B, H, W, Cout, generator=g).to(dev)
    spec = ConvSpec.dense(*nchs)
    wp = _packed_weight(w.contiguous(), spec, None)
    y = base.clone()
    shift = 1 if (use_res and B > 1) else 0
    conv_raw([_src(t, 0, c, 0, None, 0, B) for t, c in zip(xs, nchs)], wp, spec.kpad * coutpad(Cout), b, Cout if bias else 0,
             y.data_ptr(), H * W * Cout, Cout, B, H, W, Cout, 1, relu=relu,
             residual=_src(res, 0, Cout, shift, B, 0, B) if use_res else None, bpg=B // G, accumulate=acc,
             mask=_src(mask, 0, Cout, 0, None, 0, B) if use_mask else None)
    xd = torch.cat(xs, -1).double().cpu()
    wd = w.double().cpu()
    ref = torch.stack([xd[i] @ wd[(i // (B // G))][:, :, 0].T for i in range(B)])
    if bias: ref = ref + b.double().cpu()[torch.arange(B) // (B // G)][:, None, None, :]
    if use_res: ref = ref + torch.roll(res.double().cpu(), -shift, 0)
    if relu: ref = ref.clamp_min(0)
    if use_mask: ref = torch.where(mask.double().cpu() > 0, ref, torch.zeros_like(ref))
    if acc: ref = ref + base.double().cpu()
    err = ((y.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-30)).item()
    out.append((err, float(y.double().sum())))
print(json.dumps(out))
'''.replace("ROOT", repr(root))
    res = {}
    for tag, env in (("conv1p", {"BMC_CONV1P_MIN_TILES": "0"}), ("old", {"BMC_CONV1P": "0"})):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-3000:]
        res[tag] = json.loads(r.stdout.strip().splitlines()[-1])
    for i, ((e1, s1), (e0, s0)) in enumerate(zip(res["conv1p"], res["old"])):
        assert e1 < 3e-6 and e0 < 3e-6, (i, e1, e0)
        assert abs(s1 - s0) <= 1e-3 * max(1.0, abs(s0)), (i, s1, s0)


# ------------------------------------------------------------------ small frames: paired residual blocks (ops.pair_small)
def test_paired_residual_blocks_match_separate_launches():
    """BMCNet(4,128,2) at 31x56, bs 4 (configs[3]'s frame: one block's launch is 128 tiles, the pair 256): two recurrent windows
    forward + backward with the two weight-distinct residual blocks of every ParallelBlk as two-group launches (the default
    there) and as separate launches -- same losses and parameter gradients up to the Winograd / direct kernel difference."""
    dev = _gpu()
    from bmc_hip import ops
    from models.BMCNet import BMCNet
    torch.manual_seed(3)
    scale, n_c, n_b, B, H, W = 4, 128, 2, 4, 31, 56
    m = BMCNet(scale, n_c, n_b).to(dev)
    scaled_init(m, 2.0)
    g = torch.Generator().manual_seed(8)
    frames = torch.poisson(torch.full((B, 3, 2, H, W), 0.284), generator=g).to(dev)
    gt = torch.rand(B, 2, scale * H, scale * W, generator=g).to(dev)
    assert ops.pair_small(2 * B, H, W)

    def run():
        for p in m.parameters():
            p.grad = None
        z = lambda c: torch.zeros(B, c, H, W, device=dev)
        state = (z(n_c), z(n_c), z(n_c), z(2 * scale * scale))
        loss = 0
        for i in range(2):
            out = m(frames[:, i:i + 2].transpose(1, 2), *state, i == 0)
            state = tuple(out)
            loss = loss + F.mse_loss(out[-1], gt)
        loss.backward()
        return float(loss), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    la, ga = run()
    old = ops.PAIR_SMALL
    ops.PAIR_SMALL = False
    try:
        assert not ops.pair_small(2 * B, H, W)
        lb, gb = run()
    finally:
        ops.PAIR_SMALL = old
    assert abs(la - lb) <= 1e-5 * abs(lb)
    assert ga.keys() == gb.keys()
    worst = max(rel_l2(ga[k], gb[k]) for k in ga)
    print("paired vs separate: loss %.6f / %.6f, worst parameter-gradient difference %.2e" % (la, lb, worst))
    assert worst < 2e-4


@pytest.mark.parametrize("cins", [[16, 128, 16], [128, 128, 16, 16], [128, 32]])
def test_split_multi_source_weight_gradient_vs_float64(cins):
    """ops.split_wgrad on the GPU: a multi-source 3x3 convolution on LEAF parameters -- the 128-channel sources' weight gradients
    through the Winograd kernel (each into its own column window of .grad), the narrow ones through one pixel-reduction launch,
    the bias from the first -- against float64 autograd, and against the single direct launch (BMC_WINO_WGRAD off)."""
    dev = _gpu()
    from bmc_hip import ops
    from bmc_hip.ops import ConvSpec, View
    torch.manual_seed(sum(cins))
    B, H, W, Cout = 2, 13, 22, 128
    xs = [torch.randn(B, H, W, c, device=dev) for c in cins]
    w = torch.nn.Parameter(torch.randn(Cout, sum(cins), 3, 3, device=dev) * 0.05)
    b = torch.nn.Parameter(torch.randn(Cout, device=dev) * 0.1)
    go = torch.randn(B, H, W, Cout, device=dev)
    spec = ConvSpec.dense(*cins)
    ops.set_accumulate_param_grads(True)

    def grads():
        w.grad = b.grad = None
        y = ops.conv([View(x) for x in xs], w, b, spec, relu=True)
        y.backward(go)
        return w.grad.detach().clone(), b.grad.detach().clone()

    assert ops.split_wgrad(spec, [View(x).meta() for x in xs]) is not None
    gw, gb = grads()
    old = ops.WINO_WGRAD
    ops.WINO_WGRAD = False
    try:
        gw_d, gb_d = grads()
    finally:
        ops.WINO_WGRAD = old
    x64 = torch.cat([x.cpu().double() for x in xs], -1).permute(0, 3, 1, 2)
    w64 = w.detach().cpu().double().requires_grad_(True)
    b64 = b.detach().cpu().double().requires_grad_(True)
    y64 = F.relu(F.conv2d(x64, w64, b64, padding=1))
    y64.backward(go.cpu().double().permute(0, 3, 1, 2))
    rel = lambda a, r: float((a.cpu().double() - r).norm() / r.norm())
    e_w, e_b, e_d = rel(gw, w64.grad), rel(gb, b64.grad), rel(gw_d, w64.grad)
    print("sources %s: split dW %.2e db %.2e, single launch dW %.2e" % (cins, e_w, e_b, e_d))
    assert e_w < 2e-6 and e_b < 2e-6 and e_d < 2e-6
    # a second backward accumulates (gradient accumulation over micro-batches): exactly twice the first
    y = ops.conv([View(x) for x in xs], w, b, spec, relu=True)
    y.backward(go)
    assert rel(w.grad, 2 * w64.grad) < 2e-6 and rel(b.grad, 2 * b64.grad) < 2e-6


# ------------------------------------------------------------------ torch-tensor encodings (dataloader/encodings.py:16-73, 100-148)
def test_torch_encodings_match_reference_golden_bit_for_bit():
    """events_to_image_torch (bilinear with / without padding and clipping, interpolation=None) and events_to_voxel_torch on the
    GPU against the REFERENCE's outputs on the same events (tests/golden/encodings_torch.npz): images, voxel grids and the
    in-place resets of the inputs, bit for bit; plus the early-out cases."""
    dev = _gpu()
    from bmc_hip import encodings as E
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encodings_torch.npz"))
    H, W = 13, 17
    T = lambda k: torch.tensor(g[k].copy(), device=dev)
    for pad, clip in ((True, True), (True, False), (False, True)):
        a, b, c = T("xs"), T("ys"), T("ps")
        img = E.events_to_image_torch(a, b, c, sensor_size=(H, W), clip_out_of_range=clip, interpolation="bilinear", padding=pad)
        tag = "img_pad%d_clip%d" % (pad, clip)
        assert np.array_equal(img.cpu().numpy(), g[tag]), tag
        for t, k in ((a, "_xs"), (b, "_ys"), (c, "_ps")):
            assert np.array_equal(t.cpu().numpy(), g[tag + k]), tag + k
    with pytest.raises(RuntimeError):
        E.events_to_image_torch(T("xs"), T("ys"), T("ps"), sensor_size=(H, W), clip_out_of_range=False, interpolation="bilinear", padding=False)
    a, b, c = T("xi"), T("yi"), T("ps")
    assert np.array_equal(E.events_to_image_torch(a, b, c, sensor_size=(H, W)).cpu().numpy(), g["imgn"])
    assert np.array_equal(a.cpu().numpy(), g["imgn_xs"]) and np.array_equal(c.cpu().numpy(), g["imgn_ps"])
    a, b = T("xi"), T("yi")
    vox = E.events_to_voxel_torch(a, b, T("ts"), T("ps"), 5, sensor_size=(H, W))
    assert np.array_equal(vox.cpu().numpy(), g["vox"])
    assert np.array_equal(a.cpu().numpy(), g["vox_xs"]) and np.array_equal(b.cpu().numpy(), g["vox_ys"])
    a, b = T("xi"), T("yi")
    z = E.events_to_voxel_torch(a, b, torch.zeros_like(T("ts")), T("ps"), 5, sensor_size=(H, W))
    assert np.array_equal(z.cpu().numpy(), g["vox_zero_ts"]) and np.array_equal(a.cpu().numpy(), g["xi"])     # untouched inputs
    z = E.events_to_voxel_torch(T("xi")[:3].clone(), T("yi")[:3].clone(), T("ts")[:3].clone(), T("ps")[:3].clone(), 5, sensor_size=(H, W))
    assert np.array_equal(z.cpu().numpy(), g["vox_three"])


def test_torch_encodings_vs_oracle_at_sensor_size():
    """The same two encodings at 180x240 with 60 000 events (hot pixels included: one pixel receives 5 000 events) against the numpy
    restatements of the reference (pinned to its outputs by tests/test_oracle_golden_r2.py): bit-identical, run to run as well."""
    dev = _gpu()
    from bmc_hip import encodings as E
    from oracle import bmc_oracle as O
    rng = np.random.default_rng(12)
    H, W, n = 180, 240, 60000
    xs = (rng.random(n) * (W + 2) - 1).astype(np.float32)
    ys = (rng.random(n) * (H + 2) - 1).astype(np.float32)
    xs[:5000] = 100.25; ys[:5000] = 50.75
    ps = rng.standard_normal(n).astype(np.float32)
    ref = O.events_to_image_torch_np(xs.copy(), ys.copy(), ps.copy(), (H, W), interpolation="bilinear")
    outs = []
    for _ in range(2):
        a, b, c = (torch.tensor(v.copy(), device=dev) for v in (xs, ys, ps))
        outs.append(E.events_to_image_torch(a, b, c, sensor_size=(H, W), interpolation="bilinear").cpu().numpy())
    assert np.array_equal(outs[0], ref) and np.array_equal(outs[0], outs[1])
    xi, yi = np.floor(xs), np.floor(ys)
    ts = np.sort(rng.random(n).astype(np.float32) * np.float32(0.03) + np.float32(1.5))
    refv = O.events_to_voxel_torch_np(xi.copy(), yi.copy(), ts, ps.copy(), 5, (H, W))
    a, b = torch.tensor(xi.copy(), device=dev), torch.tensor(yi.copy(), device=dev)
    vox = E.events_to_voxel_torch(a, b, torch.tensor(ts, device=dev), torch.tensor(ps, device=dev), 5, sensor_size=(H, W))
    assert np.array_equal(vox.cpu().numpy(), refv)
