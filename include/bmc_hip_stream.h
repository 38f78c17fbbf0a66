/* bmc_hip_stream.h -- companion of bmc_hip.h: ONE continuous super-resolved event stream from overlapping windows.
 *
 * bmc_slot_emit_clocked (bmc_hip.h) stores every window's events on the recording's own clock.  The reference cuts a recording
 * into items of `window` events that advance by window - sliding_window, so consecutive items overlap; window i predicts item
 * i+1 and spreads its events over that item's whole span, and the concatenation of a recording's windows then carries every
 * stretch of sensor time as often as items cover it, out of time order.  The entry point below TRIMS each window, before its
 * sort, to the stretch of time that no later window covers.  It is exported by the same library (csrc/slot_emit_trimmed.hip)
 * and described, as text made by the compiler from these declarations, by bmc_stream_abi() -- the records of bmc_abi()
 * (csrc/abi.hip) -- from which bmc_hip/stream_lib.py builds its binding.  bmc_hip.h itself is unchanged by it.
 *
 * DEFINITION (the contract).  Per slot and window, with q, the event set, xs / ys / ps, the order (the exact rational
 * j / (n - 1), ties in flat emission order) and the float64 time t of every event EXACTLY as bmc_slot_emit_clocked defines them:
 *   1. TIME.   For event j (0 <= j < n) of an element with n = q events, g = gcd(j, n - 1), all in float64:
 *                tau = T0 + (T1 - T0) * (j / g) / ((n - 1) / g)    the product, then the quotient, then the sum, each rounded
 *                                                                   on its own; tau = T0 for n = 1,
 *                dt  = t_last - t_first                             one subtraction, rounded once,
 *                t   = t_first + tau * dt                           a multiply and an add, each rounded on its own: never a
 *                                                                   fused multiply-add.
 *   2. CUT.    The window emits exactly the events with t < t_cut, a float64 comparison, STRICT: an event at t_cut itself
 *              belongs to the window that starts there.  t_cut = +inf keeps everything; a NaN never compares below and keeps
 *              nothing (the host refuses it before it gets here).
 *   3. PREFIX. t is non-decreasing along the sorted window (tau is strictly increasing in the rational, the product with
 *              dt >= 0 and the sum are monotone after rounding), and equal rationals share one tau (the reduced fraction), hence
 *              one t.  So the kept events are a PREFIX of the window bmc_slot_emit_clocked would store, a run of ties is kept
 *              or dropped whole, and the kept events have the same xs / ys / ps / t, bit for bit, in the same order.  Within
 *              one element t is non-decreasing in j, so an element with n events contributes its first k(n) events,
 *                k(n) = #{ j < n : t(j, n) < t_cut },
 *              which depends on n alone: the kernels find k(n) for n = 0 .. 255 by bisection over j (at most 8 evaluations
 *              of the SAME device function that computes the stored time), once per workgroup, before they touch an element.
 *   4. COUNTS. kept = the sum of k(q) over the slot's elements, dropped = the sum of q - k(q).  *index_out = *index_in + kept
 *              ALWAYS; both capacity rules of the timed output apply to KEPT events: the event at global position g is stored
 *              when g < capacity, and a window of more than window_capacity kept events stores nothing and still advances the
 *              index by its kept count.  A window whose full count exceeds window_capacity but whose kept count fits IS stored:
 *              dropped events are never expanded into records, counted into the histograms, or given room in the scratch.
 *              *dropped = dropped (when the pointer is given), stored or not.
 *   5. DEGENERATE.  t_last == t_first: every event has t = t_first, the window is kept whole (t_first < t_cut) or dropped
 *              whole.  t_cut <= t_first + T0 * dt (the earliest time a window can hold): the window emits nothing.
 *   6. UNCLOCKED.  A slot whose clock entry has ts == NULL behaves as under bmc_slot_emit_clocked: untrimmed, with the float32
 *              column of its emit entry; *dropped = 0.
 * With cuts at the starts of the items the next windows predict, the concatenation of a recording's windows is non-decreasing in
 * t and covers every instant once; with non-overlapping spans nothing is dropped and every output byte equals
 * bmc_slot_emit_clocked's.
 * Determinism: integer keys and counts; no workgroup waits for another; no atomics on global memory (the low-digit histogram is
 * counted with integer LDS atomics: order independent); grids fixed by the arguments, the live sizes read from device memory:
 * the same bytes run after run, capturable in a graph. */
#ifndef BMC_HIP_STREAM_H
#define BMC_HIP_STREAM_H

#include "bmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BMC_SLOT_TRIM_PARTS 2       /* words of `parts` per (slot, part): the kept and the dropped events of the part */

/* The trim entry of a slot: a fifth DEVICE table of S entries, parallel to the slot, emit and clock tables and refreshed per
 * window like them. */
typedef struct bmc_slot_trim {
    double t_cut;               /* events with t < t_cut are emitted; +inf: all of them */
    long long* dropped;         /* NULL, or where the number of events the window lost to the cut goes */
} bmc_slot_trim_t;

/* bmc_slot_emit_clocked with the cut: its arguments, limits and scratch (bmc_slot_emit_timed_scratch_bytes), and `trim`
 * (8-byte aligned); `parts` holds BMC_SLOT_TRIM_PARTS x S x nparts words.  The same SIX launches on the same grids:
 *   count    (nparts, S)  builds k(0 .. 255) in LDS (thread n bisects for k(n)), then part p sums k(q) and q - k(q) over its
 *                         chunk -> parts[s][p] and parts[S * nparts + s * nparts + p], and counts the LOW digits of the kept
 *                         events only -> hist[s][p][256];
 *   scan     (S)          bmc_slot_emit_timed's kernel: the kept total -> *index_out, the comparison with window_capacity;
 *   expand   (nparts, S)  builds k() as the count launch did and scans k(q) per tile; the record of a kept event carries the
 *                         element's ORIGINAL n = q, on which its rank and its time depend.  Part 0 adds the slot's dropped
 *                         parts (integers) and stores *dropped;
 *   histogram, scan, scatter   bmc_slot_emit_timed's kernels as they are: they see a window of `kept` records.
 * Refused before any launch (-1, message in bmc_last_error): what bmc_slot_emit_clocked refuses, and a trim table that is NULL
 * or not 8-byte aligned. */
int bmc_slot_emit_trimmed(const bmc_slot_t* table, const bmc_slot_emit_timed_t* emit, const bmc_slot_clock_t* clock,
                          const bmc_slot_trim_t* trim, int S, const float* pred, int sH, int sW, int max_count, int nparts,
                          unsigned* parts, const unsigned short* rank_table, void* scratch, long long window_capacity,
                          bmc_stream_t s);

/* The ABI text of this header: fn, struct, field and const records as bmc_abi() writes them. */
const char* bmc_stream_abi(void);

#ifdef __cplusplus
}
#endif

#endif /* BMC_HIP_STREAM_H */
