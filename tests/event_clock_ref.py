"""The numpy restatement of the CLOCKED event stream (include/bmc_hip.h, bmc_slot_emit_clocked) and of the host rules around it
(the index table of a recording without ground truth, the span of every item), shared by test_event_clock_cpu.py and
test_gpu_event_clock.py: what the GPU kernel and the host functions must produce byte for byte."""
import numpy as np

from event_output_ref import emit_np
from event_times_ref import T0, T1, event_jn_np, exact_key_np

# the spans the tests use: a degenerate one, epoch seconds, sensor microseconds around 1e8, a span of one microsecond
SPANS = [(0.0, 0.0), (1.7e9, 1.7e9 + 0.033), (123456789.0, 123459837.0), (5.0e5, 5.0e5 + 1e-6)]


def tau_np(j, n):
    """tau = T0 + (T1 - T0) * (j / g) / ((n - 1) / g), g = gcd(j, n - 1), in float64 (product, quotient, sum); T0 for n = 1."""
    j, n = np.asarray(j, np.int64), np.asarray(n, np.int64)
    d = np.maximum(n - 1, 1)
    g = np.gcd(j, d)                                       # gcd(0, d) = d: the fraction 0 / 1
    return np.where(n > 1, T0 + (T1 - T0) * (j // g).astype(np.float64) / (d // g).astype(np.float64), T0)


def clock_np(tau, t_first, t_last):
    """t = t_first + tau * (t_last - t_first): numpy rounds the product and the sum separately."""
    t_first, t_last = np.float64(t_first), np.float64(t_last)
    prod = np.asarray(tau, np.float64) * (t_last - t_first)
    return t_first + prod


def emit_clocked_np(P, span, max_count=255):
    """P [2,sH,sW], span = (t_first, t_last) -> (xs int16, ys int16, ps int8, ts float64, q): the events and the order of
    event_times_ref.emit_timed_np, with float64 times on the clock."""
    assert max_count <= 255
    xs, ys, ps, q = emit_np(P, max_count)
    j, n = event_jn_np(q)
    order = np.argsort(exact_key_np(j, n), kind="stable")
    return xs[order], ys[order], ps[order], clock_np(tau_np(j, n), *span)[order], q


def lr_blocks_np(n, window, sliding_window, dataset_length=None):
    """compute_k_indices without ground truth (dataloader/h5dataset.py:197-215), one block at a time."""
    step = window - sliding_window
    L = int(n / step)
    if dataset_length is not None:
        L = min(dataset_length, L)
    rows = []
    for j in range(L):
        idx0 = step * j
        rows.append((idx0, min(idx0 + window, n - 1)))
    return np.asarray(rows, np.int64).reshape(-1, 2)


def block_spans_np(ts, index):
    """(ts[first], ts[end - 1]) per item; an empty item: ts[min(first, n - 1)] twice."""
    out = []
    for first, end in np.asarray(index).tolist():
        if end > first:
            out.append((ts[first], ts[end - 1]))
        else:
            out.append((ts[min(first, len(ts) - 1)],) * 2)
    return np.asarray(out, np.float64).reshape(-1, 2)
