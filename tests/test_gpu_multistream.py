"""Multi-stream inference on the MI355X (infer.MultiStreamSR, csrc/slots.hip): many recordings of different lengths
through one batched model, recordings joining and leaving the batch, against StreamingSR run per recording, the float64
oracle and the reference golden; the slot kernels on their own."""
import numpy as np
import pytest
import torch

from test_gpu_r2 import _gpu, load, oracle_params, rel_l2, scaled_init, _restore_math_mode  # noqa: F401
from parity_bars import CONTRACT_SR, within

pytestmark = pytest.mark.gpu

SCALE, SEQN = 4, 3


def _model(plain, n_c, n_b=1, seed=0, gain=2.0):
    from models.BMCNet import BMCNet
    from models.BMCNet_plain import BMCNet_plain
    torch.manual_seed(seed)
    m = (BMCNet_plain if plain else BMCNet)(SCALE, n_c, n_b)
    scaled_init(m, gain)
    return m


def _recordings(windows, H, W, gh, gw, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in windows:
        L = n + SEQN - 1
        out.append((torch.poisson(torch.full((L, 2, H, W), 0.4), generator=g),
                    torch.poisson(torch.full((L, 2, gh, gw), 0.1), generator=g)))
    return out


def _streaming(m, n_c, plain, frames, gts, gt_size, state_dtype=None):
    """StreamingSR per recording -> (predictions, esr_mse, bicubic_mse) per window."""
    from infer import StreamingSR
    sr = StreamingSR(m, n_c=n_c, scale=SCALE, plain=plain, state_dtype=state_dtype)
    preds, esr, bic = [], [], []
    for i in range(frames.shape[0] - SEQN + 1):
        x = frames[None, i:i + SEQN].transpose(1, 2)
        p = sr.step(x)
        preds.append(p[0].clone())
        esr.append(StreamingSR.esr_mse(p, gts[None, i + 1]).item())
        bic.append(StreamingSR.bicubic_mse(frames[None, i + 1], gts[None, i + 1], gt_size).item())
    return preds, esr, bic


def _oracle(m, n_c, plain, frames, gts, round_state=False):
    """float64 oracle per recording -> (predictions, esr_mse, bicubic_mse) per window."""
    import torch.nn.functional as F
    from oracle import bmc_oracle as O
    p = {k: v.detach().double() for k, v in oracle_params(m).items()}
    f, gt = frames.double(), gts.double()
    H, W = f.shape[-2:]
    z = lambda c: torch.zeros(1, c, H, W, dtype=torch.float64)
    st = (z(n_c),) * (1 if plain else 3) + (z(2 * SCALE * SCALE),)
    out = []
    with torch.no_grad():
        for i in range(f.shape[0] - SEQN + 1):
            x = f[None, i:i + SEQN].transpose(1, 2)
            if plain:
                res = O.plain_forward(p, x, *st, i == 0, SCALE)
            else:
                res = O.bmcnet_forward(p, x, *st, i == 0, SCALE)
            st = tuple(O.round_bf16(t) for t in res[:-1]) + (res[-1],) if round_state else res
            pred, g = res[-1], gt[None, i + 1]
            esr = pred if pred.shape[-2:] == g.shape[-2:] else O.bicubic_resize(pred, g.shape[-2:])
            base = O.bicubic_resize(f[None, i + 1], g.shape[-2:])
            out.append((pred[0], F.mse_loss(esr, g).item(), F.mse_loss(base, g).item()))
    return out


def _multi(m, n_c, plain, recs, S, graph, state_dtype=None, dev="cuda:0"):
    from infer import MultiStreamSR
    ms = MultiStreamSR(m, S, n_c=n_c, scale=SCALE, plain=plain, graph=graph, state_dtype=state_dtype, keep_predictions=True)
    hs = [ms.open(f.to(dev), g.to(dev)) for f, g in recs]
    ms.run()
    return ms, [ms.results(h) for h in hs]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


# ------------------------------------------------------------------ 1. the same as sequential evaluation
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("plain", [False, True])
def test_matches_sequential_evaluation(plain, graph):
    """5 recordings of 2-7 windows in 2 slots: recordings start in reused slots mid-run.  EventZoom-like ground truth two
    columns narrower than the prediction (the resize branch of both metrics)."""
    dev = _gpu()
    n_c, H, W = 16, 10, 16
    gh, gw = SCALE * H, SCALE * W - 2
    m = _model(plain, n_c, seed=11)
    recs = _recordings([2, 7, 3, 5, 4], H, W, gh, gw, seed=12)
    ref64 = [_oracle(m, n_c, plain, f, g) for f, g in recs]
    m.to(dev)
    ms, res = _multi(m, n_c, plain, recs, 2, graph)
    if graph:
        assert ms._graph is not None and ms.replays > 0
    worst = 0.0
    for (f, g), r, o in zip(recs, res, ref64):
        preds, esr, bic = _streaming(m, n_c, plain, f.to(dev), g.to(dev), (gh, gw))
        assert r["predictions"].shape[0] == len(preds) == len(r["esr_mse"]) == len(r["time"])
        for i in range(len(preds)):
            assert rel_l2(r["predictions"][i], preds[i]) <= 1e-5, i
            assert _rel(r["esr_mse"][i], esr[i]) <= 1e-5 and _rel(r["bicubic_mse"][i], bic[i]) <= 1e-5, i
            worst = max(worst, rel_l2(r["predictions"][i], o[i][0]))
            assert _rel(r["esr_mse"][i], o[i][1]) <= CONTRACT_SR and _rel(r["bicubic_mse"][i], o[i][2]) <= CONTRACT_SR, i
        assert all(t > 0 for t in r["time"])
    within(worst, CONTRACT_SR, CONTRACT_SR, "multi-stream predictions vs float64 oracle (%s, %s)" % (
        "plain" if plain else "BMCNet", "graph" if graph else "eager"))


def test_matches_sequential_evaluation_full_width():
    """n_c = 128 at the NFS sensor size 45x80, 4 slots."""
    dev = _gpu()
    n_c, H, W = 128, 45, 80
    m = _model(False, n_c, seed=21, gain=1.0).to(dev)
    recs = _recordings([3, 2, 4, 2, 3], H, W, SCALE * H, SCALE * W, seed=22)
    _, res = _multi(m, n_c, False, recs, 4, False)
    for (f, g), r in zip(recs, res):
        preds, esr, bic = _streaming(m, n_c, False, f.to(dev), g.to(dev), None)
        for i in range(len(preds)):
            assert rel_l2(r["predictions"][i], preds[i]) <= 1e-5, i
            assert _rel(r["esr_mse"][i], esr[i]) <= 1e-5 and _rel(r["bicubic_mse"][i], bic[i]) <= 1e-5, i


# ------------------------------------------------------------------ 2. one slot: bit-identical to StreamingSR
@pytest.mark.parametrize("plain", [False, True])
def test_one_slot_bit_identical_to_streaming(plain):
    """The init=False zero-state first window computes exactly what StreamingSR's init=True first window computes."""
    dev = _gpu()
    n_c, H, W = 16, 10, 16
    m = _model(plain, n_c, seed=31).to(dev)
    recs = _recordings([5], H, W, SCALE * H, SCALE * W, seed=32)
    _, res = _multi(m, n_c, plain, recs, 1, False)
    preds, _, _ = _streaming(m, n_c, plain, recs[0][0].to(dev), recs[0][1].to(dev), None)
    for i, p in enumerate(preds):
        assert torch.equal(res[0]["predictions"][i], p), i


# ------------------------------------------------------------------ 3. slots are independent
@pytest.mark.parametrize("graph", [False, True])
def test_slots_are_independent(graph):
    """With S fixed, a recording's predictions and metrics are bit-equal whether its neighbours carry other recordings or are
    empty, and whether it starts in a fresh slot or in one reused after another recording."""
    dev = _gpu()
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=41).to(dev)
    a, b, c, d = _recordings([4, 1, 6, 5], H, W, SCALE * H, SCALE * W - 2, seed=42)
    _, alone = _multi(m, n_c, False, [a], 3, graph)                 # slot 0, slots 1 and 2 empty
    _, crowd = _multi(m, n_c, False, [b, c, d, a], 3, graph)        # slot 0 after b (reset mid-run), c and d beside it
    x, y = alone[0], crowd[3]
    assert torch.equal(x["predictions"], y["predictions"])
    assert x["esr_mse"] == y["esr_mse"] and x["bicubic_mse"] == y["bicubic_mse"]


# ------------------------------------------------------------------ 4. the reference golden through evaluate_recordings
@pytest.mark.parametrize("graph", [False, True])
def test_reference_golden_through_evaluate_recordings(graph):
    dev = _gpu()
    from infer import evaluate_recordings
    from models.BMCNet import BMCNet
    from test_gpu_parity import _load_sd
    z = load("infer_seqn3.npz")
    scale, n_c, n_b, B, H, W, seqn, nwin, gh, gw = (int(v) for v in z["meta"])
    m = BMCNet(scale, n_c, n_b)
    _load_sd(m, z)
    m.to(dev)
    frames, gts = torch.tensor(z["frames"]).to(dev), torch.tensor(z["gts"]).to(dev)
    recs = {"sample%d" % b: (frames[b, :nwin + seqn - 1], gts[b, :nwin + seqn - 1]) for b in range(B)}
    out = evaluate_recordings(m, recs, 2, n_c=n_c, scale=scale, graph=graph, seqn=seqn, gt_size=(gh, gw), keep_predictions=True)
    for b in range(B):
        p = out["predictions"]["sample%d" % b]
        assert p.shape[0] == nwin
        for i in range(nwin):
            assert rel_l2(p[i], z["pred%d" % i][b]) < 1e-4, (b, i)
    esr = float(np.mean([float(z["esr_mse%d" % i]) for i in range(nwin)]))
    bic = float(np.mean([float(z["bicubic_mse%d" % i]) for i in range(nwin)]))
    assert abs(out["mean"]["esr_mse"] - esr) < 1e-4 * esr
    assert abs(out["mean"]["bicubic_mse"] - bic) < 1e-5 * bic
    params = sum(q.numel() for q in m.parameters()) / 1e6
    assert out["mean"]["params"] == params and set(out["results"]["time"]) == set(recs)


# ------------------------------------------------------------------ 5. bf16 state pool
@pytest.mark.parametrize("graph", [False, True])
def test_bf16_state_pool_vs_oracle_with_state_rounding(graph):
    dev = _gpu()
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=51)
    recs = _recordings([3, 5, 2], H, W, SCALE * H, SCALE * W, seed=52)
    ref = [_oracle(m, n_c, False, f.float(), g, round_state=True) for f, g in recs]
    m.to(dev)
    _, res = _multi(m, n_c, False, recs, 2, graph, state_dtype=torch.bfloat16)
    worst = max(rel_l2(r["predictions"][i], o[i][0]) for r, o in zip(res, ref) for i in range(len(o)))
    within(worst, 1e-5, CONTRACT_SR, "multi-stream, state pool in bf16, vs the oracle with state rounding")


def test_commit_rounds_like_torch_bf16():
    """bmc_slot_commit into a bf16 pool == tensor.to(torch.bfloat16), bit for bit: ties both ways, NaN, infinities, the
    largest finite values, subnormals."""
    dev = _gpu()
    from bmc_hip import slots
    S, H, W, C = 2, 4, 8, 16
    n = 2 * H * W * C
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int64).to(torch.int32)
    special = torch.tensor([0x3F808000, 0x3F818000, 0x3F80C000, 0x7F7FFFFF, 0x7F7F8000, 0xFF7F8000, 0x7F800000, 0xFF800000,
                            0x00008000, 0x00018000, 0x80000000, 0x00000001], dtype=torch.int64)
    bits[:special.numel()] = special.to(torch.int32)
    src = bits.view(torch.float32)
    src = torch.where(torch.isnan(src), torch.zeros_like(src), src).view(S, H, W, C).to(dev)
    pool = torch.zeros(1, S, H, W, C, dtype=torch.bfloat16, device=dev)
    table = slots.SlotTable(S, dev)
    e = table.host()
    dummy = torch.zeros(2 * SEQN * H * W, device=dev)
    e["frames"] = dummy.data_ptr()
    e["flags"] = slots.ACTIVE
    table.upload()
    pred = torch.zeros(S, 2, SCALE * H, SCALE * W, device=dev)
    slots.commit(table, [src.permute(0, 3, 1, 2)], pool, pred.clone(), pred)
    want = src.to(torch.bfloat16)
    assert torch.equal(pool[0].view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------ 6. the slot kernels on their own
@pytest.mark.parametrize("bf16", [False, True])
def test_stage_and_commit_bit_exact(bf16):
    dev = _gpu()
    from bmc_hip import slots
    S, H, W, C, nfeat, L = 4, 6, 10, 16, 3, 7
    sH, sW = SCALE * H, SCALE * W
    g = torch.Generator().manual_seed(61)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    frames = [rnd(L, 2, H, W) for _ in range(S)]
    flags = [slots.ACTIVE, slots.ACTIVE | slots.RESET, 0, slots.ACTIVE]
    win = [2, 0, 0, 4]
    pool = rnd(nfeat, S, H, W, C).to(torch.bfloat16 if bf16 else torch.float32)
    pool0 = pool.clone()
    feat = torch.full((nfeat, S, H, W, C), 7.0, device=dev) if bf16 else pool
    pred = rnd(S, 2, sH, sW)
    pred0 = pred.clone()
    x = torch.full((S, 2, SEQN, H, W), 5.0, device=dev)
    table = slots.SlotTable(S, dev)
    e = table.host()
    for s in range(S):
        if flags[s]:
            e[s]["frames"] = frames[s].data_ptr() + 4 * win[s] * 2 * H * W
        e[s]["flags"] = flags[s]
    table.upload()
    slots.stage(table, x, pool, feat, pred)
    for s in range(S):
        zero = not (flags[s] & slots.ACTIVE) or bool(flags[s] & slots.RESET)
        want_x = frames[s][win[s]:win[s] + SEQN].transpose(0, 1) if flags[s] & slots.ACTIVE else torch.zeros_like(x[s])
        assert torch.equal(x[s], want_x), s
        assert torch.equal(feat[:, s], torch.zeros_like(feat[:, s]) if zero else pool0[:, s].float()), s
        assert torch.equal(pred[s], torch.zeros_like(pred[s]) if zero else pred0[s]), s
    # commit: active slots only; the prediction also to `keep`
    srcs = [rnd(S, H, W, C).permute(0, 3, 1, 2) for _ in range(nfeat)]
    new_pred = rnd(S, 2, sH, sW)
    keep = torch.zeros(2, sH, sW, device=dev)
    e = table.host()
    for s in range(S):
        if flags[s]:
            e[s]["frames"] = frames[s].data_ptr()
        e[s]["flags"] = flags[s]
    e[3]["keep"] = keep.data_ptr()
    table.upload()
    before_pool, before_pred = pool.clone(), pred.clone()
    slots.commit(table, srcs, pool, new_pred, pred)
    for s in range(S):
        if flags[s] & slots.ACTIVE:
            for k in range(nfeat):
                assert torch.equal(pool[k, s], srcs[k][s].permute(1, 2, 0).to(pool.dtype)), (s, k)
            assert torch.equal(pred[s], new_pred[s]), s
        else:
            assert torch.equal(pool[:, s], before_pool[:, s]) and torch.equal(pred[s], before_pred[s]), s
    assert torch.equal(keep, new_pred[3])


@pytest.mark.parametrize("case", ["same", "eventzoom"])
def test_metrics_vs_float64_oracle_and_reproducible(case):
    dev = _gpu()
    from bmc_hip import slots
    from oracle import bmc_oracle as O
    H, W = (10, 16) if case == "same" else (31, 56)
    sH, sW = SCALE * H, SCALE * W
    gh, gw = (sH, sW) if case == "same" else (124, 222)
    S, L = 3, 4
    g = torch.Generator().manual_seed(71)
    frames = [torch.poisson(torch.full((L, 2, H, W), 0.5), generator=g).to(dev) for _ in range(S)]
    gts = [torch.poisson(torch.full((L, 2, gh, gw), 0.2), generator=g).to(dev) for _ in range(S)]
    pred = (torch.rand(S, 2, sH, sW, generator=g) * 0.6).to(dev)
    nparts = slots.metric_parts(gh, gw)
    out = torch.full((S, nparts, 2), -1.0, dtype=torch.float64, device=dev)
    win = [0, 2, 1]
    table = slots.SlotTable(S, dev)

    def run():
        e = table.host()
        for s in range(S):
            e[s]["frames"] = frames[s].data_ptr() + 4 * win[s] * 2 * H * W
            e[s]["gt"] = gts[s][win[s] + 1].data_ptr()
            e[s]["result"] = out[s].data_ptr()
            e[s]["flags"] = slots.ACTIVE
        table.upload()
        slots.metrics(table, pred, H, W, gh, gw, nparts)
        return slots.sum_parts(out)

    r1, r2 = run(), run()
    assert torch.equal(r1, r2)
    n = 2 * gh * gw
    for s in range(S):
        gt = gts[s][win[s] + 1].double().cpu()
        p = pred[s].double().cpu()
        esr = p if case == "same" else O.bicubic_resize(p, (gh, gw))
        base = O.bicubic_resize(frames[s][win[s] + 1].double().cpu(), (gh, gw))
        assert _rel(r1[s, 0].item() / n, float(((esr - gt) ** 2).mean())) < 1e-5, s
        assert _rel(r1[s, 1].item() / n, float(((base - gt) ** 2).mean())) < 1e-5, s


# ------------------------------------------------------------------ 7. one launch each per window
def test_one_launch_each_per_window():
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    n_c, H, W = 16, 10, 16
    m = _model(False, n_c, seed=81).to(dev)
    for S in (2, 4):
        ms = MultiStreamSR(m, S, n_c=n_c, scale=SCALE)
        for f, g in _recordings([3] * S, H, W, SCALE * H, SCALE * W, seed=82):
            ms.open(f.to(dev), g.to(dev))
        for _ in range(3):
            before = dict(slots.LAUNCHES)
            assert ms.step()
            assert {k: slots.LAUNCHES[k] - before[k] for k in before} == {"stage": 1, "commit": 1, "metrics": 1}
        assert not ms.step()
    ms = MultiStreamSR(m, 4, n_c=n_c, scale=SCALE, graph=True)
    for f, g in _recordings([8] * 4, H, W, SCALE * H, SCALE * W, seed=83):
        ms.open(f.to(dev), g.to(dev))
    for _ in range(3):                   # two eager windows, the capture with the first replay
        ms.step()
    for k in range(3):
        before = dict(slots.LAUNCHES)
        ms.step()
        assert ms.replays == 2 + k and slots.LAUNCHES == before
    with torch.no_grad():                # a parameter update: the next window captures afresh
        m.neuro.conv_o.bias.add_(0.01)
    ms.run()
    assert slots.LAUNCHES["stage"] == before["stage"] + 1 and ms.replays == 6


def test_open_refuses_other_sizes_and_short_recordings():
    dev = _gpu()
    from infer import MultiStreamSR
    m = _model(False, 16).to(dev)
    ms = MultiStreamSR(m, 2, n_c=16, scale=SCALE)
    (f, g), = _recordings([2], 10, 16, 40, 64, seed=91)
    ms.open(f.to(dev), g.to(dev))
    (f2, g2), = _recordings([2], 12, 16, 48, 64, seed=92)
    with pytest.raises(ValueError):
        ms.open(f2.to(dev), g2.to(dev))
    with pytest.raises(ValueError):
        ms.open(f[:SEQN - 1].to(dev), g[:SEQN - 1].to(dev))
    with pytest.raises(ValueError):
        ms.open(f.to(dev), g.to(dev), gt_size=(40, 62))
