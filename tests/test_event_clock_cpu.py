"""CPU checks of deployment recordings (infer.MultiStreamSR without ground truth, events on the sensor's clock;
csrc/slot_emit_timed.hip, bmc_slot_emit_clocked): the index table of a recording without ground truth against the restated rule
and the reference's recorded tables, the spans of the items, the properties of the reduced-fraction time that the float64
column rests on, the argument checks, and the layout of bmc_slot_clock_t.  Every comparison is exact."""
import os
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

from event_clock_ref import SPANS, block_spans_np, clock_np, emit_clocked_np, lr_blocks_np, tau_np
from event_times_ref import emit_timed_np, event_jn_np, exact_key_np, times_np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


# ------------------------------------------------------------------ index tables without ground truth
@pytest.mark.parametrize("n,window,sliding,length", [(1024, 256, 128, None), (1000, 256, 128, None), (400, 64, 48, 20),
                                                     (400, 64, 48, None), (257, 256, 0, None), (2049, 2048, 1024, None)])
def test_index_table_without_ground_truth_equals_the_rule(n, window, sliding, length):
    from bmc_hip.encodings import event_window_indices
    ts = np.sort(np.random.default_rng(n).uniform(0, 1, n))
    lr_index, gt_index = event_window_indices(ts, None, window, sliding, 4, dataset_length=length)
    want = lr_blocks_np(n, window, sliding, length)
    assert gt_index is None and lr_index.dtype == np.int64 and np.array_equal(lr_index, want)
    assert len(want) == (int(n / (window - sliding)) if length is None else min(length, int(n / (window - sliding))))
    assert want[-1, 1] <= n - 1 and (want[:, 1] - want[:, 0] <= window).all()


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_index_table_without_ground_truth_begins_with_the_golden_table(tag):
    """The reference's own event_indices (recorded WITH ground truth) are the first rows: nothing is cut by HR coverage (c:
    the HR stream ends early -- the table with ground truth has 15 rows, the reference's event_indices 25, all of them here)."""
    from bmc_hip.encodings import event_window_indices
    z = _golden("event_windows")
    window, sliding, scale, length = (int(v) for v in z[tag + "_cfg"])
    kw = dict(window=window, sliding_window=sliding, scale=scale, dataset_length=None if length < 0 else length)
    lr_index, none = event_window_indices(z[tag + "_lr_ts"], None, **kw)
    gold = z[tag + "_lr_index"]
    assert none is None and len(lr_index) >= len(gold) and np.array_equal(lr_index[:len(gold)], gold)
    with_gt = event_window_indices(z[tag + "_lr_ts"], z[tag + "_gt_ts"], **kw)[0]
    assert np.array_equal(lr_index[:len(with_gt)], with_gt)            # today's table, possibly followed by further rows
    if tag == "c":
        assert len(with_gt) < len(lr_index) == len(gold)


def test_index_table_without_ground_truth_keeps_the_refusals():
    from bmc_hip.encodings import event_window_indices
    ts = np.linspace(0, 1, 600)
    for mode in ("time", "frame"):
        with pytest.raises(ValueError):
            event_window_indices(ts, None, 256, 128, mode=mode)
    with pytest.raises(ValueError):
        event_window_indices(ts[:100], None)                            # no block
    with pytest.raises(ValueError):
        event_window_indices(ts.reshape(2, -1), None, 256, 128)


# ------------------------------------------------------------------ spans of the items
def test_event_block_spans_on_hand_made_tables():
    """A one-event item, an empty item inside, an empty item at the very end (clamped to the last event) and a clamped tail
    block (end = n - 1: the last event is never used)."""
    from bmc_hip.encodings import event_block_spans
    ts = np.array([10.0, 11.0, 11.0, 12.5, 1.7e9, 1.7e9 + 1e-6, 1.7e9 + 2.0])
    index = np.array([[0, 4], [2, 3], [3, 3], [7, 7], [4, 6], [0, 7]])
    want = np.array([[10.0, 12.5], [11.0, 11.0], [12.5, 12.5], [1.7e9 + 2.0] * 2, [1.7e9, 1.7e9 + 1e-6], [10.0, 1.7e9 + 2.0]])
    for col in (ts, torch.from_numpy(ts)):
        got = event_block_spans(col, index)
        assert got.dtype == np.float64 and got.shape == (6, 2) and got.tobytes() == want.tobytes()
    assert event_block_spans(ts, index).tobytes() == block_spans_np(ts, index).tobytes()
    assert event_block_spans(ts, torch.from_numpy(index)).tobytes() == want.tobytes()
    for bad in (np.array([[0, 8]]), np.array([[3, 2]]), np.array([[-1, 2]]), np.array([[0.0, 2.0]]), np.array([0, 2])):
        with pytest.raises(ValueError):
            event_block_spans(ts, bad)
    with pytest.raises(ValueError):
        event_block_spans(ts[:0], np.array([[0, 0]]))


def test_event_block_spans_on_the_reference_tables():
    from bmc_hip.encodings import event_block_spans, event_window_indices
    z = _golden("event_windows")
    for tag in "abc":
        window, sliding, scale, length = (int(v) for v in z[tag + "_cfg"])
        ts = z[tag + "_lr_ts"]
        index = event_window_indices(ts, None, window, sliding, scale, dataset_length=None if length < 0 else length)[0]
        spans = event_block_spans(ts, index)
        assert spans.tobytes() == block_spans_np(ts, index).tobytes()
        assert (spans[:, 1] >= spans[:, 0]).all() and spans[0, 0] == ts[0] and spans[-1, 1] == ts[index[-1, 1] - 1]


# ------------------------------------------------------------------ the reduced-fraction time
def _all_jn():
    n, j = np.meshgrid(np.arange(1, 256), np.arange(255), indexing="ij")
    ok = j < n
    return j[ok], n[ok]


def test_tau_has_one_value_per_rational_and_increases_strictly():
    j, n = _all_jn()
    tau = tau_np(j, n)
    assert tau.dtype == np.float64
    by_rational = {}
    for jj, nn, t in zip(j.tolist(), n.tolist(), tau.tolist()):
        by_rational.setdefault(Fraction(jj, nn - 1) if nn > 1 else Fraction(0), set()).add(t)
    assert len(by_rational) == 19693 and all(len(v) == 1 for v in by_rational.values())          # one tau per rational
    values = [next(iter(by_rational[f])) for f in sorted(by_rational)]
    assert (np.diff(np.asarray(values)) > 0).all() and values[0] == 0.01 and values[-1] == 1.0    # strictly increasing
    # the unreduced float64 expression is NOT single valued: this is why the fraction is reduced
    raw = np.where(n > 1, 0.01 + (1.0 - 0.01) * j.astype(np.float64) / np.maximum(n - 1, 1), 0.01)
    split = {}
    for jj, nn, t in zip(j.tolist(), n.tolist(), raw.tolist()):
        split.setdefault(Fraction(jj, nn - 1) if nn > 1 else Fraction(0), set()).add(t)
    assert sum(len(v) > 1 for v in split.values()) == 925


def test_float32_of_tau_is_the_timed_outputs_time():
    j, n = _all_jn()
    assert tau_np(j, n).astype(np.float32).tobytes() == times_np(j, n).tobytes()                  # every (j, n), n <= 255
    z = _golden("event_times")
    for k in range(4):                                                 # ... and the times of the golden count images
        q = z["q%d" % k].astype(np.float32)
        ts32 = emit_timed_np(q)[3]
        ts64 = emit_clocked_np(q, (0.0, 1.0))[3]
        jj, nn = event_jn_np(z["q%d" % k])
        order = np.argsort(exact_key_np(jj, nn), kind="stable")
        assert ts64.tobytes() == tau_np(jj, nn)[order].tobytes()       # span (0, 1): t = 0 + tau * 1 = tau
        assert ts64.astype(np.float32).tobytes() == ts32.tobytes()
        # the reference's own float32 linspace: the bound test_event_times_cpu derives (1e-6), position by position
        assert (np.abs(z["cloud%d" % k][:, 2].astype(np.float64) - ts64) <= 1e-6).all()


@pytest.mark.parametrize("span", SPANS + [(-3.5, 7.25), (1e15, 1e15 + 1.0)])
def test_clock_time_is_non_decreasing_along_the_sorted_window(span):
    """All (j, n) in the order of the exact rational: t never decreases, starts at t_first + 0.01 dt and ends on t_last."""
    j, n = _all_jn()
    order = np.argsort(exact_key_np(j, n), kind="stable")
    t = clock_np(tau_np(j, n), *span)[order]
    assert t.dtype == np.float64 and (np.diff(t) >= 0).all()
    assert t[-1] == np.float64(span[0]) + (np.float64(span[1]) - np.float64(span[0]))             # tau = 1: t_last
    assert t[0] == np.float64(span[0]) + 0.01 * (np.float64(span[1]) - np.float64(span[0]))
    if span[1] > span[0] + 1e-3:
        assert t[-1] > t[0]


def test_restatement_small_example():
    P = np.array([[[2.0, 0.0], [1.0, 3.0]], [[0.0, 0.0], [0.0, 5.0]]], np.float32)
    xs, ys, ps, ts, q = emit_clocked_np(P, (1000.0, 1100.0))
    wx, wy, wp, wt, _ = emit_timed_np(P)
    assert xs.tobytes() == wx.tobytes() and ys.tobytes() == wy.tobytes() and ps.tobytes() == wp.tobytes()
    assert ts.dtype == np.float64 and ts.tolist() == [1001.0] * 4 + [1000.0 + (0.01 + 0.99 * 1 / 4) * 100.0] + \
        [1000.0 + (0.01 + 0.99 * 1 / 2) * 100.0] * 2 + [1000.0 + (0.01 + 0.99 * 3 / 4) * 100.0] + [1100.0] * 3


# ------------------------------------------------------------------ argument checks (no device needed)
def _session(**kw):
    from infer import MultiStreamSR
    return MultiStreamSR(torch.nn.Identity(), 2, n_c=16, scale=4, **kw)


def _clocked():
    return _session(emit_events=True, event_times="linear")


def _event_args(gt=True):
    cols = lambda n: (torch.ones(n, dtype=torch.int16), torch.ones(n, dtype=torch.int16), torch.ones(n, dtype=torch.float64))
    a = dict(lr=cols(100), lr_index=np.stack([20 * np.arange(4), 20 * np.arange(4) + 40], 1), lr_size=(10, 16))
    if gt:
        a.update(gt=cols(400), gt_index=np.stack([80 * np.arange(4), 80 * np.arange(4) + 160], 1), gt_size=(40, 64))
    return a


def test_recordings_without_ground_truth_pass_the_host_checks():
    """Everything that can be checked on the host passes; only the device is missing."""
    with pytest.raises(ValueError, match="GPU"):
        _session().open(torch.zeros(4, 2, 10, 16))
    with pytest.raises(ValueError, match="GPU"):
        _session().open(torch.zeros(4, 2, 10, 16), None)
    with pytest.raises(ValueError, match="GPU"):
        _session().open_events(**_event_args(gt=False))
    with pytest.raises(ValueError, match="GPU"):
        _session().open_events(_event_args()["lr"], None, _event_args()["lr_index"], None, (10, 16), None)
    with pytest.raises(ValueError, match="gt_size without"):
        _session().open(torch.zeros(4, 2, 10, 16), None, gt_size=(40, 64))
    with pytest.raises(ValueError, match=r"frames \[L,2,H,W\]"):
        _session().open(torch.zeros(4, 3, 10, 16))


@pytest.mark.parametrize("drop", ["gt", "gt_index", "gt_size", ("gt", "gt_index"), ("gt", "gt_size"), ("gt_index", "gt_size")])
def test_ground_truth_arguments_are_all_given_or_all_none(drop):
    a = _event_args()
    for k in (drop,) if isinstance(drop, str) else drop:
        a[k] = None
    ms = _session()
    with pytest.raises(ValueError, match="all given or all None"):
        ms.open_events(**a)
    assert not ms.sched.pending() and ms._size is None


def test_event_recording_without_ground_truth():
    from infer import EventRecording
    a = _event_args(gt=False)
    r = EventRecording(a["lr"], lr_index=a["lr_index"], lr_size=a["lr_size"])
    assert r.gt is None and r.gt_index is None and r.gt_size is None and r.lr_size == (10, 16)
    assert EventRecording(a["lr"], None, a["lr_index"], None, a["lr_size"], None) == r


@pytest.mark.parametrize("kind", ["open", "open_events", "open_events_ts"])
def test_spans_need_a_timed_session(kind):
    spans = np.array([[0.0, 1.0]] * 4)
    for ms in (_session(), _session(emit_events=True)):
        with pytest.raises(ValueError, match="event_times='linear'"):
            if kind == "open":
                ms.open(torch.zeros(4, 2, 10, 16), spans=spans)
            elif kind == "open_events":
                ms.open_events(spans=spans, **_event_args())
            else:
                ms.open_events(lr_ts=np.arange(100.0), **_event_args())
        assert not ms.sched.pending() and ms._size is None


@pytest.mark.parametrize("bad,match", [
    (np.array([[0.0, 1.0]] * 3), "spans must be"), (np.array([0.0, 1.0] * 4), "spans must be"),
    (np.array([[0.0, 1.0]] * 3 + [[2.0, 1.0]]), "t_last >= t_first"), (np.array([[0.0, 1.0]] * 3 + [[0.0, np.inf]]), "finite"),
    (np.array([[np.nan, 1.0]] + [[0.0, 1.0]] * 3), "finite"), (np.array([["a", "b"]] * 4), "spans must be"),
])
def test_bad_spans_are_refused(bad, match):
    for kind in ("open", "open_events"):
        ms = _clocked()
        with pytest.raises(ValueError, match=match):
            ms.open(torch.zeros(4, 2, 10, 16), spans=bad) if kind == "open" else ms.open_events(spans=bad, **_event_args())
        assert not ms.sched.pending() and ms._size is None


def test_lr_ts_checks():
    a = _event_args(gt=False)
    with pytest.raises(ValueError, match="not both"):
        _clocked().open_events(lr_ts=np.arange(100.0), spans=np.array([[0.0, 1.0]] * 4), **a)
    for bad in (np.arange(99.0), np.arange(100.0).astype(np.float32), np.arange(100), np.zeros((100, 1)), list(range(100))):
        with pytest.raises(ValueError, match="lr_ts must be"):
            _clocked().open_events(lr_ts=bad, **a)
    with pytest.raises(ValueError, match="t_last >= t_first"):         # a column that runs backwards
        _clocked().open_events(lr_ts=-np.arange(100.0), **a)
    for good in (np.arange(100.0), torch.arange(100.0, dtype=torch.float64)):
        with pytest.raises(ValueError, match="GPU"):                   # a good one passes the host checks
            _clocked().open_events(lr_ts=good, **a)
    with pytest.raises(ValueError, match="GPU"):
        _clocked().open(torch.zeros(4, 2, 10, 16), spans=[[0.0, 0.0], [1.0, 2.0], [2, 3], [1.7e9, 1.7e9]])


def test_counts_to_events_span_refusals():
    from bmc_hip.encodings import counts_to_events
    with pytest.raises(ValueError, match="times='linear'"):
        counts_to_events(torch.zeros(1, 2, 8, 8), spans=[[0.0, 1.0]])
    with pytest.raises(ValueError, match="spans must be"):
        counts_to_events(torch.zeros(2, 2, 8, 8), times="linear", spans=[[0.0, 1.0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        counts_to_events(torch.zeros(1, 2, 8, 8), times="linear", spans=[[0.0, 1.0]])


def test_slots_emit_clocked_refusals():
    from bmc_hip import slots
    pred, parts, scratch = torch.zeros(2, 2, 8, 8), torch.zeros(2, dtype=torch.int32), torch.zeros(8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no clock entries"):
        slots.emit_clocked(types.SimpleNamespace(S=2, emit=True, timed=True, clock=False), pred, 255, 1, parts, scratch, 10)
    table = types.SimpleNamespace(S=2, emit=True, timed=True, clock=True)
    with pytest.raises(ValueError, match="no timed emit entries"):
        slots.emit_clocked(types.SimpleNamespace(S=2, emit=True, timed=False, clock=True), pred, 255, 1, parts, scratch, 10)
    for bad in (0, 256, 1.0, True):                                    # the argument checks of emit_timed
        with pytest.raises(ValueError, match="max_count"):
            slots.emit_clocked(table, pred, bad, 1, parts, scratch, 10)
    for bad in (0, -1, 2.0, (1 << 28) + 1):
        with pytest.raises(ValueError, match="window_capacity"):
            slots.emit_clocked(table, pred, 255, 1, parts, scratch, bad)
    with pytest.raises(ValueError, match="GPU tensor"):
        slots.emit_clocked(table, pred, 255, 1, parts, scratch, 10)
    with pytest.raises(ValueError, match="clock=True needs timed=True"):
        slots.SlotTable(2, "cpu", emit=True, clock=True)
    assert slots.EMIT_TIMED_LAUNCHES == 0 and slots.EMIT_TIMED_KERNELS == 6


def test_tool_knows_the_options():
    src = open(os.path.join(ROOT, "tools", "multistream_infer.py")).read()
    assert '"--no-gt"' in src and '"--sensor-clock"' in src


# ------------------------------------------------------------------ C ABI
def test_library_exports_slot_emit_clocked():
    from bmc_hip import lib
    assert "bmc_slot_emit_clocked" in lib.EXPORTS and lib.has_symbol("bmc_slot_emit_clocked")


def test_slot_clock_struct_layout_matches_header():
    import abi_ref
    from bmc_hip import slots
    fields = ["t_first", "t_last", "ts"]
    structs = abi_ref.compiled_header()[0]
    size, compiled = structs["bmc_slot_clock_t"]
    dt = slots.SLOT_CLOCK_DTYPE
    assert [size] + [compiled[f][0] for f in fields] + [compiled["t_first"][1], compiled["ts"][1], structs["bmc_slot_emit_timed_t"][0],
                                                        structs["bmc_slot_emit_t"][0]] == \
        [dt.itemsize] + [dt.fields[f][1] for f in fields] + [8, 8, slots.SLOT_EMIT_TIMED_DTYPE.itemsize, slots.SLOT_EMIT_DTYPE.itemsize]
    assert dt.names == tuple(fields) and dt.itemsize == 24
    assert dt.fields["t_first"][0] == np.dtype("<f8") and dt.fields["t_last"][0] == np.dtype("<f8")
    assert slots.SLOT_EMIT_TIMED_DTYPE.itemsize == 56 and slots.SLOT_EMIT_DTYPE.itemsize == 48        # the existing layouts stay
