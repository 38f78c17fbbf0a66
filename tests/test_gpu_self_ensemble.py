"""Self-ensemble of multi-stream inference on the MI355X (infer.MultiStreamSR(self_ensemble=K); csrc/slots.hip): the oriented
gather of bmc_slot_stage and the merge of bmc_slot_commit alone, bit for bit against the numpy restatement
(self_ensemble_ref.py), and whole sessions against a plain session that runs the K pre-oriented copies of every recording."""
import numpy as np
import pytest
import torch

import self_ensemble_ref as R
from test_gpu_r2 import _gpu, scaled_init, _restore_math_mode  # noqa: F401

pytestmark = pytest.mark.gpu

SEQN = 3
NAN = float("nan")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _orient_t(t, o):
    """O_o of a tensor [..., 2, H, W], by torch.flip and a channel swap."""
    dims = [d for d, on in ((-1, o & 1), (-2, o & 2), (-3, o & 4)) if on]
    return torch.flip(t, dims).contiguous() if dims else t.contiguous()


# ------------------------------------------------------------------ 1. the stage kernel alone
def test_stage_orients_the_frames():
    dev = _gpu()
    from bmc_hip import slots
    S, H, W, C, L, sH, sW = 8, 5, 7, 4, 6, 10, 14
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    frames = [rnd(L, 2, H, W) for _ in range(S)]
    win = [0, 1, 2, 3, 0, 1, 2, 3]
    flags = [slots.ACTIVE, slots.ACTIVE | slots.RESET, slots.ACTIVE, 0, slots.ACTIVE | slots.RESET, slots.ACTIVE, slots.ACTIVE, slots.ACTIVE]
    for codes in (list(range(8)), [0] * 8):
        pool = rnd(1, S, H, W, C)
        pool0 = pool.clone()
        pred = rnd(S, 2, sH, sW)
        pred0 = pred.clone()
        x = torch.full((S, 2, SEQN, H, W), 5.0, device=dev)
        table = slots.SlotTable(S, dev)
        e = table.host()
        for s in range(S):
            if flags[s]:
                e[s]["frames"] = frames[s].data_ptr() + 4 * win[s] * 2 * H * W
            e[s]["flags"] = flags[s] | codes[s] << slots.ORIENT_SHIFT          # (an empty slot with a code stays empty)
        table.upload()
        slots.stage(table, x, pool, pool, pred)
        for s in range(S):
            active, zero = bool(flags[s] & slots.ACTIVE), not flags[s] & slots.ACTIVE or bool(flags[s] & slots.RESET)
            w = frames[s][win[s]:win[s] + SEQN].cpu().numpy()
            want = R.orient(w, codes[s]).transpose(1, 0, 2, 3) if active else np.zeros((2, SEQN, H, W), np.float32)
            assert x[s].cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes(), (codes[s], s)
            if active and not codes[s]:                     # what the stage test of the plain kernel expects
                assert torch.equal(x[s], frames[s][win[s]:win[s] + SEQN].transpose(0, 1)), s
            assert torch.equal(pool[:, s], torch.zeros_like(pool[:, s]) if zero else pool0[:, s]), s
            assert torch.equal(pred[s], torch.zeros_like(pred[s]) if zero else pred0[s]), s


# ------------------------------------------------------------------ 2. the commit kernel alone
GUARD = 64          # floats of NaN on either side of every buffer


def _guarded(n, dev, dtype=torch.float32):
    """-> (whole, view): `view` is n elements in the middle of `whole`, whose other 2 x GUARD elements are NaN."""
    whole = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n]


GROUPS = {"K8": (8, list(range(8))), "K2": (2, [0, 1] * 4), "K4": (4, [0, 1, 2, 3] * 2), "K8_shuffled": (8, [0, 6, 3, 7, 1, 5, 2, 4]),
          "K4_shuffled": (4, [0, 7, 5, 2, 0, 4, 4, 1])}


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("sH,sW", [(10, 14), (24, 32)])
def test_commit_merges_each_group(sH, sW, group, bf16):
    dev = _gpu()
    from bmc_hip import slots
    K, codes = GROUPS[group]
    S, H, W, C, nfeat = 8, 3, 4, 4, 2
    pred_n, feat_n = 2 * sH * sW, H * W * C
    g = torch.Generator().manual_seed(7 + sW)
    rnd = lambda n: (torch.randn(n, generator=g) * 10.0 ** torch.randint(-2, 3, (n,), generator=g).float()).to(dev)
    bufs = {"src": _guarded(S * pred_n, dev), "pred_pool": _guarded(S * pred_n, dev),
            "pool": _guarded(nfeat * S * feat_n, dev, torch.bfloat16 if bf16 else torch.float32)}
    bufs["src"][1].copy_(rnd(S * pred_n))
    keeps = {s: _guarded(pred_n, dev) for s in range(0, S, K)}
    feats = [_guarded(S * feat_n, dev) for _ in range(nfeat)]
    for _, v in feats:
        v.copy_(rnd(S * feat_n))
    dummy = torch.zeros(2 * SEQN * H * W, device=dev)
    src = bufs["src"][1].view(S, 2, sH, sW)
    src0 = src.clone()
    everything = [w for w, _ in list(bufs.values()) + list(keeps.values()) + feats]
    before = [w.clone() for w in everything]
    table = slots.SlotTable(S, dev)
    e = table.host()
    for s in range(S):
        e[s]["frames"] = dummy.data_ptr()
        e[s]["flags"] = slots.ACTIVE | codes[s] << slots.ORIENT_SHIFT
        if s % K == 0:
            e[s]["flags"] |= K << slots.GROUP_SHIFT
            e[s]["pad_"] = sW
            e[s]["keep"] = keeps[s][1].data_ptr()
    table.upload()
    pool = bufs["pool"][1].view(nfeat, S, H, W, C)
    slots.commit(table, [v.view(S, H, W, C).permute(0, 3, 1, 2) for _, v in feats], pool, src, bufs["pred_pool"][1].view(S, 2, sH, sW))
    torch.cuda.synchronize()
    assert _same_bits(bufs["pred_pool"][1].view(S, 2, sH, sW), src0)            # every slot's OWN prediction goes on
    for k, (_, v) in enumerate(feats):
        assert torch.equal(pool[k], v.view(S, H, W, C).to(pool.dtype)), k
    p0 = src0.cpu().numpy()
    for s in range(S):
        if s % K:
            assert _same_bits(src[s], src0[s]), s                                # member rows are only read
            continue
        want = R.merge(p0[s:s + K], codes[s:s + K])
        assert src[s].cpu().numpy().tobytes() == want.tobytes(), s
        assert keeps[s][1].cpu().numpy().tobytes() == want.tobytes(), s
    for w, b in zip(everything, before):                                         # nothing outside the buffers was written
        wi = w.view(torch.int16 if w.dtype == torch.bfloat16 else torch.int32)
        bi = b.view(wi.dtype)
        assert torch.equal(wi[:GUARD], bi[:GUARD]) and torch.equal(wi[-GUARD:], bi[-GUARD:])


def test_commit_without_a_group_ignores_the_row_length():
    """K = 0 with a pad_, a K that is no group size, a group that runs past the table: the plain copy for every slot."""
    dev = _gpu()
    from bmc_hip import slots
    S, H, W, C, sH, sW = 4, 3, 4, 4, 6, 8
    g = torch.Generator().manual_seed(9)
    src = torch.randn(S, 2, sH, sW, generator=g).to(dev)
    src0 = src.clone()
    pred = torch.zeros_like(src)
    pool = torch.zeros(1, S, H, W, C, device=dev)
    feat = torch.randn(S, H, W, C, generator=g).to(dev)
    dummy = torch.zeros(2 * SEQN * H * W, device=dev)
    table = slots.SlotTable(S, dev)
    e = table.host()
    e["frames"], e["flags"], e["pad_"] = dummy.data_ptr(), slots.ACTIVE, sW
    e[1]["flags"] |= 3 << slots.GROUP_SHIFT
    e[2]["flags"] |= 4 << slots.GROUP_SHIFT                 # slots 2 .. 5 of 4
    e[3]["flags"] |= 2 << slots.GROUP_SHIFT
    table.upload()
    slots.commit(table, [feat.permute(0, 3, 1, 2)], pool, src, pred)
    assert torch.equal(src, src0) and torch.equal(pred, src0) and torch.equal(pool[0], feat)


# ------------------------------------------------------------------ 3. sessions
def _model(plain, n_c, scale, seed):
    from models.BMCNet import BMCNet
    from models.BMCNet_plain import BMCNet_plain
    torch.manual_seed(seed)
    m = (BMCNet_plain if plain else BMCNet)(scale, n_c, 1)
    scaled_init(m, 2.0)
    return m


def _recordings(windows, H, W, gh, gw, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.poisson(torch.full((n + SEQN - 1, 2, H, W), 0.4), generator=g),
             torch.poisson(torch.full((n + SEQN - 1, 2, gh, gw), 0.1), generator=g)) for n in windows]


def _merged_from_copies(res, K):
    """The results of a recording's K oriented copies -> the restated merge of every window [n,2,sH,sW] (numpy)."""
    p = np.stack([r["predictions"].cpu().numpy() for r in res])                 # [K,n,2,sH,sW]
    return np.stack([R.merge(np.ascontiguousarray(p[:, i]), list(range(K))) for i in range(p.shape[1])])


CASES = [(plain, graph, size, 8) for plain in (False, True) for graph in (False, True) for size in ((6, 8, 4), (5, 7, 2))] + \
        [(True, graph, (5, 7, 2), K) for graph in (False, True) for K in (2, 4)]


@pytest.mark.parametrize("plain,graph,size,K", CASES)
def test_session_equals_the_oriented_copies_merged(plain, graph, size, K):
    dev = _gpu()
    from infer import MultiStreamSR
    H, W, scale = size
    n_c, sH, sW = 16, scale * H, scale * W
    m = _model(plain, n_c, scale, seed=3).to(dev)
    recs = [(f.to(dev), g.to(dev)) for f, g in _recordings([4, 3], H, W, sH, sW, seed=4 + K)]
    kw = dict(n_c=n_c, scale=scale, plain=plain, graph=graph, keep_predictions=True)
    a = MultiStreamSR(m, 2 * K, self_ensemble=K, **kw)
    ha = [a.open(f, g) for f, g in recs]
    a.run()
    b = MultiStreamSR(m, 2 * K, **kw)
    hb = [[b.open(_orient_t(f, j), g if j == 0 else None) for j in range(K)] for f, g in recs]
    b.run()
    if graph:
        assert a._graph is not None and a.replays == b.replays > 0
    for h, copies, (f, g) in zip(ha, hb, recs):
        ra, rb = a.results(h), [b.results(c) for c in copies]
        want = _merged_from_copies(rb, K)
        assert ra["predictions"].shape[0] == f.shape[0] - SEQN + 1 == len(ra["esr_mse"]) == len(ra["time"])
        assert ra["predictions"].cpu().numpy().tobytes() == want.tobytes()
        assert not torch.equal(ra["predictions"], rb[0]["predictions"])          # the merge acted
        assert ra["bicubic_mse"] == rb[0]["bicubic_mse"]
        for i, v in enumerate(ra["esr_mse"]):
            ref = R.esr_mse(want[i], g[i + 1].cpu().numpy())
            print("esr_mse window %d: %.17g, restated %.17g" % (i, v, ref))
            assert abs(v - ref) <= 1e-12 * ref, i


@pytest.mark.parametrize("graph", [False, True])
def test_option_off_is_the_plain_session(graph):
    dev = _gpu()
    from infer import MultiStreamSR
    H, W, scale, n_c = 6, 8, 4, 16
    m = _model(False, n_c, scale, seed=13).to(dev)
    recs = [(f.to(dev), g.to(dev)) for f, g in _recordings([3, 2, 4], H, W, scale * H, scale * W - 2, seed=14)]
    out = []
    for kw in ({}, {"self_ensemble": None}):
        ms = MultiStreamSR(m, 2, n_c=n_c, scale=scale, graph=graph, keep_predictions=True, **kw)
        hs = [ms.open(f, g) for f, g in recs]
        ms.run()
        out.append([ms.results(h) for h in hs])
    for x, y in zip(*out):
        assert torch.equal(x["predictions"], y["predictions"]) and x["esr_mse"] == y["esr_mse"] and x["bicubic_mse"] == y["bicubic_mse"]


@pytest.mark.parametrize("graph,hot", [(False, False), (True, True)])
def test_event_backed_ensemble_encodes_each_window_once(graph, hot):
    """An event-backed ensemble session == the frame-backed one on the encoded (and, with hot_filter, filtered) frames; the
    window is encoded and filtered once for the whole group, and stage and commit stay one launch each."""
    dev = _gpu()
    from bmc_hip import slots
    from infer import MultiStreamSR
    from test_gpu_event_slots import _dev, _encode_frames
    from test_gpu_hot_filter import GH, GW, H_, W_, HF, SCALE, _session_recordings
    n_c, K = 16, 4
    m = _model(True, n_c, SCALE, seed=23).to(dev)
    recs = _session_recordings()[:3]
    kw = dict(n_c=n_c, scale=SCALE, plain=True, graph=graph, keep_predictions=True, self_ensemble=K)
    gts = [_encode_frames(gt, gi, GH, GW, dev) for _, _, gt, gi, _ in recs]
    by_frames = MultiStreamSR(m, 2 * K, **kw)
    hf = [by_frames.open(torch.tensor(f["frames"]).to(dev) if hot else _encode_frames(lr, li, H_, W_, dev), g)
          for (lr, li, _, _, f), g in zip(recs, gts)]
    by_frames.run()
    by_events = MultiStreamSR(m, 2 * K, hot_filter=HF if hot else None, **kw)
    he = [by_events.open_events(_dev(lr, dev), _dev(gt, dev), li, gi, (H_, W_), (GH, GW)) for lr, li, gt, gi, _ in recs]
    n0 = (slots.ENCODE_LAUNCHES, slots.HOT_LAUNCHES, slots.LAUNCHES["stage"], slots.LAUNCHES["commit"])
    windows = 0
    for _ in range(2):                                     # eager windows (in graph mode the third one is captured)
        assert by_events.step()
        windows += 1
    n1 = (slots.ENCODE_LAUNCHES, slots.HOT_LAUNCHES, slots.LAUNCHES["stage"], slots.LAUNCHES["commit"])
    assert [y - x for x, y in zip(n0, n1)] == [windows, windows if hot else 0, windows, windows]
    by_events.run()
    for x, y in zip(he, hf):
        rx, ry = by_events.results(x), by_frames.results(y)
        assert torch.equal(rx["predictions"], ry["predictions"]) and rx["predictions"].shape[0] > 0
        assert rx["esr_mse"] == ry["esr_mse"] and rx["bicubic_mse"] == ry["bicubic_mse"]


@pytest.mark.parametrize("graph", [False, True])
def test_outputs_are_those_of_the_merged_prediction_and_reproducible(graph):
    dev = _gpu()
    from bmc_hip.encodings import counts_to_events, counts_to_voxel, render_event_counts
    from infer import MultiStreamSR
    H, W, scale, n_c, K, bins = 6, 8, 4, 16, 4, 3
    m = _model(False, n_c, scale, seed=33).to(dev)
    recs = [(f.to(dev), g.to(dev)) for f, g in _recordings([3, 4], H, W, scale * H, scale * W, seed=34)]
    runs = []
    for _ in range(2):
        ms = MultiStreamSR(m, 2 * K, n_c=n_c, scale=scale, graph=graph, keep_predictions=True, emit_events=True, voxel_bins=bins,
                           render=("esr",), self_ensemble=K)
        hs = [ms.open(f * 3.0, g) for f, g in recs]
        ms.run()
        runs.append([ms.results(h) for h in hs])
    for r, r2 in zip(*runs):
        p = r["predictions"]
        xs, ys, ps, index = counts_to_events(p)
        assert int(index[-1]) > 0 and torch.equal(r["sr_index"], index)
        assert all(torch.equal(x, y) for x, y in zip(r["sr_events"], (xs, ys, ps)))
        assert torch.equal(r["voxels"], counts_to_voxel(p, bins))
        assert torch.equal(r["images"]["esr"], render_event_counts(p, round=True))
        assert _same_bits(p, r2["predictions"]) and r["esr_mse"] == r2["esr_mse"] and torch.equal(r["voxels"], r2["voxels"])
        assert all(torch.equal(x, y) for x, y in zip(r["sr_events"], r2["sr_events"]))
        assert torch.equal(r["images"]["esr"], r2["images"]["esr"])
