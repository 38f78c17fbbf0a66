"""The numpy restatement of the TIMED event stream (include/bmc_hip.h, bmc_slot_emit_timed), shared by
test_event_times_cpu.py and test_gpu_event_times.py: what the GPU kernels must produce byte for byte."""
import numpy as np

from event_output_ref import emit_np

T0, T1 = 0.01, 1.0                   # BMC_EVENT_T0 / BMC_EVENT_T1: linspace(c/bins + 1/(100*bins), (c+1)/bins, n), bins = 1, c = 0


def event_jn_np(q):
    """q [2,sH,sW] -> (j, n) per emitted event in flat emission order: event j of its element's n."""
    n_el = q[q > 0].astype(np.int64)                       # C order, as emit_np visits the elements
    n = np.repeat(n_el, n_el)
    j = np.arange(len(n), dtype=np.int64) - np.repeat(np.cumsum(n_el) - n_el, n_el)
    return j, n


def times_np(j, n):
    """t = float32(T0 + (T1 - T0) * j / (n - 1)) in float64, rounded once; T0 for n = 1."""
    j, n = np.asarray(j, np.float64), np.asarray(n, np.float64)
    return np.where(n > 1, T0 + (T1 - T0) * j / np.maximum(n - 1, 1), T0).astype(np.float32)


def exact_key_np(j, n):
    """floor(j * 2^40 / (n - 1)) in int64 (0 for n = 1): equal for equal rationals, and distinct rationals with denominators
    <= 254 (at least 1 / (254 * 253) apart) differ by far more than 1."""
    j, n = np.asarray(j, np.int64), np.asarray(n, np.int64)
    return np.where(n > 1, (j << 40) // np.maximum(n - 1, 1), 0)


def emit_timed_np(P, max_count=255):
    """P [2,sH,sW] -> (xs int16, ys int16, ps int8, ts float32, q): the events of emit_np with their times, sorted by the exact
    rational j / (n - 1); equal rationals keep the flat emission order (a stable sort)."""
    assert max_count <= 255
    xs, ys, ps, q = emit_np(P, max_count)
    j, n = event_jn_np(q)
    order = np.argsort(exact_key_np(j, n), kind="stable")
    return xs[order], ys[order], ps[order], times_np(j, n)[order], q
