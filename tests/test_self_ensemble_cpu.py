"""CPU checks of the self-ensemble of multi-stream inference (infer.MultiStreamSR(self_ensemble=K)): the numpy restatement of
the orientations, the scheduler's expansion of groups into slots, the table entries of a group, and the refusals."""
import numpy as np
import pytest
import torch

import self_ensemble_ref as R
from infer import MultiStreamSR, SlotScheduler


# ------------------------------------------------------------------ the orientations
def test_orientations_are_distinct_involutions():
    img = np.arange(2 * 5 * 7, dtype=np.float32).reshape(2, 5, 7)
    seen = []
    for o in range(8):
        a = R.orient(img, o)
        assert np.array_equal(R.orient(a, o), img), o
        c, y, x = 1, 3, 2                                   # one element, by the contract's formula
        assert a[c, y, x] == img[c ^ (o >> 2), 4 - y if o & 2 else y, 6 - x if o & 1 else x], o
        seen.append(a.tobytes())
    assert len(set(seen)) == 8
    assert np.array_equal(R.orient(img, 1), img[:, :, ::-1]) and np.array_equal(R.orient(img, 2), img[:, ::-1])
    assert np.array_equal(R.orient(img, 4), img[::-1])


def test_orientation_order_is_the_encoder_flip_order():
    """Bits 0..2 of the code are horizontal, vertical, polarity, as bits 0..2 of the sequence encoder's `flips`."""
    from bmc_hip import slots
    assert (slots.ORIENT_H, slots.ORIENT_V, slots.ORIENT_P) == (R.H_BIT, R.V_BIT, R.P_BIT) == (1, 2, 4)
    assert slots.ORIENT_SHIFT == 2 and slots.GROUP_SHIFT == 8 and slots.GROUP_SIZES == (2, 4, 8)
    assert not (7 << slots.ORIENT_SHIFT | 15 << slots.GROUP_SHIFT) & (slots.ACTIVE | slots.RESET)


def test_merge_is_a_sequential_float32_sum():
    rng = np.random.default_rng(3)
    p = (rng.standard_normal((4, 2, 3, 5)) * 10.0 ** rng.integers(-3, 4, (4, 2, 3, 5))).astype(np.float32)
    codes = [0, 3, 5, 6]
    m = R.merge(p, codes)
    u = [R.orient(p[j], codes[j]) for j in range(4)]
    want = np.float32(0.25) * np.float32(np.float32(np.float32(u[0] + u[1]) + u[2]) + u[3])
    assert m.dtype == np.float32 and np.array_equal(m, want)
    assert not np.array_equal(m, (np.float32(0.25) * (u[3] + u[2] + u[1] + u[0])).astype(np.float32))    # the order matters


# ------------------------------------------------------------------ groups of slots
def test_group_expansion():
    s = SlotScheduler(2)
    a, b, c = s.add(2), s.add(1), s.add(2)
    plans = []
    while True:
        p = s.plan()
        if p is None:
            break
        plans.append(SlotScheduler.expand(p, 4))
    member = lambda h, i, reset: [(h, i, reset, j) for j in range(4)]
    assert plans == [
        member(a, 0, True) + member(b, 0, True),
        member(a, 1, False) + member(c, 0, True),           # b ended: its four slots are free at once and reset together
        [None] * 4 + member(c, 1, False),                   # a ended, nothing queued: four empty slots
    ]
    assert SlotScheduler.expand([(a, 0, True), None], 1) == [(a, 0, True, 0), None]


class _Table:
    """What _fill needs of a SlotTable, on the host."""
    events = emit = clock = hot = voxel = False
    render = 0

    def __init__(self, S):
        from bmc_hip import slots
        self.entries = np.zeros(S, slots.SLOT_DTYPE)

    def host(self):
        self.entries[:] = 0
        return self.entries


@pytest.mark.parametrize("K", [2, 4, 8])
def test_fill_writes_leader_and_member_entries(K):
    from bmc_hip import slots
    H, W, gh, gw, scale, S = 5, 7, 10, 14, 2, 2 * K
    ms = MultiStreamSR(torch.nn.Identity(), S, n_c=4, scale=scale, keep_predictions=True, self_ensemble=K)
    assert len(ms.sched.slots) == 2 and ms.S == S
    ms._size = (H, W, gh, gw)
    table = _Table(S)
    ms._bufs = {"table": table}
    recs = []
    for L in (4, 5):
        r = dict(frames=torch.zeros(L, 2, H, W), gts=torch.zeros(L, 2, gh, gw), n=L - 2, steps=[], device="cpu",
                 keep=torch.zeros(L - 2, 2, scale * H, scale * W), sse=torch.zeros(L - 2, 1, 2, dtype=torch.float64))
        ms._recs[ms.sched.add(r["n"])] = r
        recs.append(r)
    for window in range(2):
        ms._fill(ms.sched.plan())
        ms._steps.append(None)
        e = table.entries
        for g, r in enumerate(recs):
            lead = e[g * K]
            assert lead["frames"] == r["frames"].data_ptr() + 4 * window * 2 * H * W
            assert lead["gt"] == r["gts"][window + 1].data_ptr() and lead["keep"] == r["keep"][window].data_ptr()
            assert lead["result"] == r["sse"][window].data_ptr()
            assert lead["flags"] == slots.ACTIVE | (slots.RESET if window == 0 else 0) | K << 8
            assert lead["pad_"] == scale * W
            for j in range(1, K):
                m = e[g * K + j]
                assert m["frames"] == lead["frames"] and m["gt"] == m["keep"] == m["result"] == 0 and m["pad_"] == 0
                assert m["flags"] == slots.ACTIVE | (slots.RESET if window == 0 else 0) | j << 2
            assert r["steps"] == list(range(window + 1))                        # one step per window, not one per member


def test_entries_without_the_option_are_unchanged():
    """self_ensemble=None: no new bit, pad_ 0 -- the entries a session wrote before the option existed."""
    from bmc_hip import slots
    ms = MultiStreamSR(torch.nn.Identity(), 3, n_c=4, scale=2, self_ensemble=None)
    ms._size = (5, 7)
    table = _Table(3)
    ms._bufs = {"table": table}
    r = dict(frames=torch.zeros(3, 2, 5, 7), n=1, steps=[], device="cpu", keep=None)
    ms._recs[ms.sched.add(1)] = r
    ms._fill(ms.sched.plan())
    e = table.entries
    assert e[0]["flags"] == slots.ACTIVE | slots.RESET and e[0]["pad_"] == 0 and e[0]["frames"] == r["frames"].data_ptr()
    assert not e[1:].tobytes().strip(b"\0")


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("K", [0, 1, 3, 6, 16, True, 2.0, "4"])
def test_group_size_is_checked(K):
    with pytest.raises(ValueError, match="self_ensemble must be None, 2, 4 or 8"):
        MultiStreamSR(torch.nn.Identity(), 16, self_ensemble=K)


@pytest.mark.parametrize("S,K", [(3, 2), (6, 4), (12, 8), (1, 2)])
def test_slots_must_be_a_multiple_of_the_group(S, K):
    with pytest.raises(ValueError, match="slots must be a multiple of self_ensemble"):
        MultiStreamSR(torch.nn.Identity(), S, self_ensemble=K)


def test_evaluate_recordings_passes_the_option_on():
    from infer import evaluate_recordings
    with pytest.raises(ValueError, match="slots must be a multiple of self_ensemble"):
        evaluate_recordings(torch.nn.Identity(), {}, 6, self_ensemble=4)
