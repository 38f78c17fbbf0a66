"""Host side of training from raw event columns (event_dataset.py), no GPU: sequence_plan, noise_events and the numpy
restatement of bmc_seq_encode against what the reference's own SequenceDataset returned (tests/golden/event_train.npz, written by
tests/golden/make_golden_event_train.py); lengths and sharding; argument checks; the C ABI."""
import os
import random

import numpy as np
import pytest
import torch

import event_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, CASES = R.load_golden()


def _cols(side):
    return tuple(G["%s_%s" % (side, c)] for c in ("xs", "ys", "ps"))


# ------------------------------------------------------------------ the golden file itself
def test_golden_covers_the_cases_the_sampling_has():
    assert any(any(c["paused"]) for c in CASES.values())
    assert any(c["augment"] and c["flips"] == 7 for c in CASES.values())
    assert any(c["augment"] and c["flips"] == 0 for c in CASES.values())
    for key in ("augment", "pause", "noise_level", "step"):          # each one on and off
        assert {c[key] is None for c in CASES.values()} == {True, False}, key
    assert {c["step"] for c in CASES.values()} >= {None, 3}
    assert os.path.getsize(R.GOLDEN) <= 300 * 1024


# ------------------------------------------------------------------ sequence_plan, the restatement
@pytest.mark.parametrize("name", sorted(CASES))
def test_sequence_plan_matches_reference(name):
    """The seed, the items, the paused flags and the flips of the reference's sequence, and the state `random` is left in."""
    from event_dataset import sequence_plan
    c = CASES[name]
    random.seed(c["rs"])
    seed, items, paused, flips = sequence_plan(c["i"], len(G["lr_index"]), c["L"], c["step"], c["augment"], c["pause"])
    assert (seed, items, paused, flips) == (c["seed"], c["items"], c["paused"], c["flips"])
    assert random.random() == c["next"]
    rng = random.Random(c["rs"])                                    # ... and on a generator of the caller's
    assert sequence_plan(c["i"], len(G["lr_index"]), c["L"], c["step"], c["augment"], c["pause"], rng=rng) == (seed, items, paused, flips)
    assert rng.random() == c["next"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_reference_frames(name):
    from event_dataset import noise_events, sequence_plan
    c = CASES[name]
    seed, items, paused, flips = sequence_plan(c["i"], len(G["lr_index"]), c["L"], c["step"], c["augment"], c["pause"],
                                               rng=random.Random(c["rs"]))
    H, W, gh, gw = G["size"].tolist()
    noise = None if c["noise_level"] is None else noise_events(int(G["window"]), (H, W), seed, c["noise_level"])
    inp, gt = R.encode_sample(_cols("lr"), _cols("gt"), G["lr_index"][items], G["gt_index"][items], flips, paused, (H, W), (gh, gw),
                              noise)
    assert inp.dtype == gt.dtype == np.float32
    assert np.array_equal(inp, c["inp"]) and np.array_equal(gt, c["gt"])
    for t, p in enumerate(paused):
        assert not p or (not inp[t].any() and gt[t].any())           # a paused item keeps its ground truth


def test_noise_events_match_reference_and_leave_the_global_generator():
    from event_dataset import noise_events
    H, W = G["size"].tolist()[:2]
    n = 0
    for c in CASES.values():
        if c["noise_level"] is None:
            continue
        torch.manual_seed(1234)
        before = torch.get_rng_state()
        xs, ys, ps = noise_events(int(G["window"]), (H, W), c["seed"], c["noise_level"])
        assert torch.equal(torch.get_rng_state(), before)
        assert (xs.dtype, ys.dtype, ps.dtype) == (np.int16, np.int16, np.int8)
        assert len(xs) == int(int(G["window"]) * c["noise_level"]) == c["noise"].shape[1]
        assert np.array_equal(np.stack([xs, ys, ps.astype(np.int16)]), c["noise"])
        n += 1
    assert n >= 3
    assert [len(a) for a in noise_events(128, (H, W), 5, 0.0)] == [0, 0, 0]


def test_pause_draws_degenerate_under_augmentation():
    """Kept, not fixed: augment_event re-seeds `random` in every item, so every pause draw of a sequence is the second draw
    after random.seed(seed + 2) -- (0.6, 0.3) then alternates or never pauses, whatever L; without augmentation the chain is a
    chain."""
    from event_dataset import sequence_plan
    c = CASES["pause_degenerate"]
    assert c["paused"] == [False, True, False, True, False, True] and CASES["pause_degenerate_all"]["paused"] == [False, True, True, True]
    aug = (G["mechanisms"].tolist(), G["probs"].tolist())
    for rs in range(40):
        rng = random.Random(rs)
        seed, items, paused, _ = sequence_plan(0, 64, 12, None, aug, (0.6, 0.3), rng=rng)
        u = random.Random(seed + 2)
        u.random()
        u = u.random()
        want = [False] + [0.3 <= u < 0.6 and t % 2 == 0 or (u < 0.3) for t in range(11)]
        assert paused == want, (rs, u)
        k = np.cumsum([0] + [not p for p in paused[1:]])
        assert items == k.tolist()
    chains = {tuple(sequence_plan(0, 64, 12, None, None, (0.5, 0.5), rng=random.Random(rs))[2]) for rs in range(40)}
    assert len(chains) > 20


def test_sequence_plan_arguments():
    from event_dataset import sequence_plan
    with pytest.raises(ValueError, match="does not fit"):
        sequence_plan(0, 8, 9)
    assert sequence_plan(0, 9, 9, rng=random.Random(0))[1] == list(range(9))
    with pytest.raises(IndexError):
        sequence_plan(1, 9, 9)
    with pytest.raises(IndexError):
        sequence_plan(-1, 20, 4)
    assert sequence_plan(5, 20, 4, 3, rng=random.Random(0))[1] == [15, 16, 17, 18]       # (20 - 4) // 3 + 1 = 6 sequences
    with pytest.raises(IndexError):
        sequence_plan(6, 20, 4, 3)
    with pytest.raises(ValueError, match="positive"):
        sequence_plan(0, 20, 4, 0)
    with pytest.raises(ValueError, match="augment"):
        sequence_plan(0, 20, 4, augment="Horizontal")
    with pytest.raises(ValueError, match="pause"):
        sequence_plan(0, 20, 4, pause=0.5)
    # a mechanism the reference does not know is skipped, its probability with it
    assert sequence_plan(0, 20, 4, augment=(["Rotate", "Polarity"], [1.0, 1.0]), rng=random.Random(0))[3] == 4


# ------------------------------------------------------------------ lengths and sharding (no GPU: the tables only)
def _set_with_lengths(lengths, **kw):
    """An EventTrainSet whose recordings are only their lengths (what __len__, locate and batches read)."""
    from event_dataset import EventTrainSet
    ts = EventTrainSet(**kw)
    for n in lengths:
        ts._recs.append(dict(lr_index=np.zeros((n, 2), np.int64), gt_index=np.zeros((n, 2), np.int64)))
        ts._ends.append(len(ts) + (n - ts.L) // ts.step_size + 1)
    return ts


def test_lengths_and_locate():
    ts = _set_with_lengths([24, 9, 40], L=9, step_size=4)
    per = [(24 - 9) // 4 + 1, 1, (40 - 9) // 4 + 1]
    assert len(ts) == sum(per) == 13
    assert [ts.locate(k) for k in (0, 3, 4, 5, 12)] == [(0, 0), (0, 3), (1, 0), (2, 0), (2, 7)]
    with pytest.raises(IndexError):
        ts.locate(13)
    assert len(_set_with_lengths([24], L=9)) == 2                    # step_size None: L
    r, seed, items, paused, flips = ts.plan(12, rng=random.Random(3))
    assert r == 2 and items == list(range(28, 37)) and not any(paused) and flips == 0


@pytest.mark.parametrize("n_items,world,bs", [(45, 1, 2), (45, 4, 2), (49, 4, 3), (12, 8, 1)])
def test_batches_shard_like_distributed_sampler(n_items, world, bs):
    from torch.utils.data.distributed import DistributedSampler
    ts = _set_with_lengths([n_items], L=5, step_size=1)
    n = len(ts)
    per_rank = -(-n // world)
    shares = []
    for rank in range(world):
        g = torch.Generator().manual_seed(7)
        b = ts.batches(bs, shuffle=True, drop_last=False, generator=g, rank=rank, world=world)
        flat = [v for part in b for v in part]
        assert len(flat) == per_rank and all(len(p) == bs for p in b[:-1]) and 1 <= len(b[-1]) <= bs
        ds = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=True, seed=7)
        assert flat == list(ds)                                      # the same permutation, padding and stride
        shares.append(flat)
        g = torch.Generator().manual_seed(7)
        dropped = ts.batches(bs, generator=g, rank=rank, world=world)
        assert dropped == [p for p in b if len(p) == bs]
    allv = [v for s in shares for v in s]
    assert set(allv) == set(range(n)) and len(allv) == per_rank * world
    if n % world == 0:
        assert len(set(allv)) == len(allv)                           # disjoint
    assert ts.batches(bs, shuffle=False, drop_last=False, rank=0, world=world)[0][0] == 0
    with pytest.raises(ValueError):
        ts.batches(bs, rank=world, world=world)
    with pytest.raises(ValueError):
        ts.batches(0)


# ------------------------------------------------------------------ argument checks that need no GPU
def test_train_set_arguments():
    from event_dataset import EventTrainSet, MAX_ITEMS
    with pytest.raises(ValueError, match="L <= 32"):
        EventTrainSet(L=MAX_ITEMS + 1)
    with pytest.raises(ValueError, match="2 <= L"):
        EventTrainSet(L=1)
    with pytest.raises(ValueError, match="step_size"):
        EventTrainSet(step_size=0)
    ts = EventTrainSet(L=4, add_noise=0.1, window=128)
    assert ts.n_noise == 12 and len(ts) == 0
    lr = tuple(torch.tensor(c) for c in _cols("lr"))
    gt = tuple(torch.tensor(c) for c in _cols("gt"))
    H, W, gh, gw = G["size"].tolist()
    good = dict(lr=lr, gt=gt, lr_index=G["lr_index"], gt_index=G["gt_index"], lr_size=(H, W), gt_size=(gh, gw))
    with pytest.raises(ValueError, match="int16, int16, float64"):
        ts.add_recording(**dict(good, lr=(lr[0], lr[1], lr[2].float())))
    with pytest.raises(ValueError, match="three tensors"):
        ts.add_recording(**dict(good, gt=gt[:2]))
    with pytest.raises(ValueError, match="outside the 2048 events"):
        ts.add_recording(**dict(good, lr_index=G["lr_index"] + 1000))
    with pytest.raises(ValueError, match="first > end"):
        ts.add_recording(**dict(good, gt_index=G["gt_index"][:, ::-1]))
    with pytest.raises(ValueError, match="integer"):
        ts.add_recording(**dict(good, lr_index=G["lr_index"].astype(np.float64)))
    with pytest.raises(ValueError, match="rows"):
        ts.add_recording(**dict(good, gt_index=G["gt_index"][:-1]))
    with pytest.raises(ValueError, match="fewer than one sequence"):
        ts.add_recording(**dict(good, lr_index=G["lr_index"][:3], gt_index=G["gt_index"][:3]))
    with pytest.raises(ValueError, match="at most 7680 wide"):
        ts.add_recording(**dict(good, gt_size=(gh, 7681)))
    with pytest.raises(ValueError, match="GPU tensors"):
        ts.add_recording(**good)                                     # everything else is in order: the columns are on the host
    assert len(ts) == 0 and ts._size is None


# ------------------------------------------------------------------ C ABI
def test_library_exports_seq_encode():
    from bmc_hip import lib
    assert "bmc_seq_encode" in lib.EXPORTS and lib.has_symbol("bmc_seq_encode")


def test_seq_sample_struct_layout_matches_header():
    import abi_ref
    import event_dataset as E
    from bmc_hip import encodings
    fields = E.SEQ_SAMPLE_DTYPE.names
    structs, constants = abi_ref.compiled_header()
    size, compiled = structs["bmc_seq_sample_t"]
    dt = E.SEQ_SAMPLE_DTYPE
    assert [size, constants["BMC_SEQ_MAX_ITEMS"]] + [compiled[f][0] for f in fields] == [dt.itemsize, E.MAX_ITEMS] + [dt.fields[f][1] for f in fields]
    assert dt.itemsize == encodings.SEQ_SAMPLE_BYTES
    assert dt.fields["lr_range"][0].shape == dt.fields["gt_range"][0].shape == (E.MAX_ITEMS, 2)
