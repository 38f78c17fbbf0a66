"""The numpy restatement of the CONTINUOUS event stream (include/bmc_hip_stream.h, bmc_slot_emit_trimmed) and of the host rule
around it (the cut of every window), shared by test_event_stream_cpu.py and test_gpu_event_stream.py: the clocked window of
event_clock_ref.emit_clocked_np, then keep = ts < t_cut -- what the GPU kernel must produce byte for byte."""
import numpy as np

from event_clock_ref import clock_np, emit_clocked_np, tau_np


def emit_trimmed_np(P, span, t_cut, max_count=255):
    """P [2,sH,sW], span = (t_first, t_last), t_cut -> (xs, ys, ps, ts, dropped): the events of the clocked window with
    ts < t_cut (strictly), in its order, and how many were cut off.  The kept events are a prefix of the sorted window."""
    xs, ys, ps, ts, _ = emit_clocked_np(P, span, max_count)
    keep = ts < np.float64(t_cut)
    k = int(keep.sum())
    assert keep[:k].all() and not keep[k:].any()
    return xs[:k], ys[:k], ps[:k], ts[:k], len(ts) - k


def time_np(j, n, span):
    """The float64 clock time of event j of an element's n events."""
    return clock_np(tau_np(j, n), *span)


def kept_brute_np(n, span, t_cut):
    """k(n) = #{ j < n : t(j, n) < t_cut }, counted."""
    return int((time_np(np.arange(n), np.full(n, n), span) < np.float64(t_cut)).sum()) if n else 0


def kept_bisect_np(n, span, t_cut):
    """k(n) as the kernels find it: at most 8 evaluations of the time, the answer bracketed in [lo, hi]."""
    lo, hi, evaluations = 0, n, 0
    for _ in range(8):
        if lo < hi:
            mid = (lo + hi) >> 1
            evaluations += 1
            if time_np(mid, n, span) < np.float64(t_cut):
                lo = mid + 1
            else:
                hi = mid
    assert lo == hi and evaluations <= 8
    return lo


def cuts_np(spans, n_windows):
    """Window i predicts item i+1 and is cut at spans[i+2][0]; the last window (or i+2 >= L) at +inf."""
    L = len(spans)
    return np.array([spans[i + 2][0] if i + 2 < L and i + 1 < n_windows else np.inf for i in range(n_windows)], np.float64)


def half_overlapping_spans(L, t0, step):
    """Items of two steps each that advance by one: the reference's blocks (window = 2048 events, advancing by 1024)."""
    first = np.float64(t0) + np.float64(step) * np.arange(L)
    return np.stack([first, first + 2.0 * np.float64(step)], 1)
