// Continuous event output of multi-stream inference (MultiStreamSR(emit_events=True, event_times="linear", continuous=True)):
// the clocked stream of slot_emit_timed.hip with every window TRIMMED to the events before t_cut, the start of the item the
// next window predicts (include/bmc_hip_stream.h states the contract, bmc_slot_emit_trimmed).  The windows of a recording
// overlap by half, so about half of a window's events are dropped -- BEFORE the sort: they are never expanded into records,
// counted into a histogram or given room in the scratch.
//
// The time of an event is non-decreasing in j inside an element, so an element with n events keeps its first k(n); k depends
// on n alone.  The count and the expand kernel each open with the table keep[256] in LDS: thread n finds k(n) by bisection
// over j with clock_time(), the very function the scatter kernel stores times with -- the kept set and the stored times cannot
// disagree.  After that an element with q events contributes keep[q]: everything else is slot_emit_timed.hip's algorithm, and
// the first scan, the histogram, the second scan and the scatter launch ARE its kernels (slot_emit_k.h, EmitTimedPlan).
// The same six launches and grids; no workgroup waits for another, no atomics on global memory.
#include "bmc_hip_stream.h"
#include "slot_emit_k.h"

namespace {

// k(n) = #{ j < n : clock_time(j, n) < t_cut } of slot s; n for a slot that is not clocked (it is not trimmed)
__device__ __forceinline__ unsigned kept_of(const bmc_slot_clock_t* clock, const bmc_slot_trim_t* trim, int s, unsigned n) {
    if (gld<double*>(&clock[s].ts) == nullptr) return n;
    const double t_first = gld<double>(&clock[s].t_first);
    const double dt = gld<double>(&clock[s].t_last) - t_first;
    const double t_cut = gld<double>(&trim[s].t_cut);
    unsigned lo = 0u, hi = n;                                         // the answer is in [lo, hi]: at most 256 values, 8 halvings
    for (int it = 0; it < 8; ++it) {
        if (lo < hi) {
            const unsigned mid = (lo + hi) >> 1;
            if (clock_time(t_first, dt, mid, n) < t_cut) lo = mid + 1u;
            else hi = mid;
        }
    }
    return lo;
}

// an element's q -> the events it keeps; qs (null, or TILE bytes of LDS) <- the q the tile's elements had before
struct KeptEvents {
    const unsigned char* keep;
    unsigned char* qs;
    __device__ __forceinline__ void operator()(unsigned (&q)[4], int e) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (qs) qs[e + k] = (unsigned char)q[k];
            q[k] = keep[q[k]];
        }
    }
};

// grid (nparts, S): emit_timed_count_kernel on the kept events; parts[s][p] <- the part's kept, dparts[s][p] <- its dropped events
__global__ __launch_bounds__(EMT) void emit_trimmed_count_kernel(const bmc_slot_t* __restrict__ table,
                                                                 const bmc_slot_emit_timed_t* __restrict__ emit,
                                                                 const bmc_slot_clock_t* __restrict__ clock,
                                                                 const bmc_slot_trim_t* __restrict__ trim,
                                                                 const float* __restrict__ pred, int n, int chunk, int vec, float mc,
                                                                 const unsigned short* __restrict__ rank,
                                                                 unsigned* __restrict__ parts, unsigned* __restrict__ dparts,
                                                                 unsigned* __restrict__ hist, int hrows) {
    __shared__ unsigned wsum[NW], wdrop[NW];
    __shared__ unsigned lh[256];
    __shared__ unsigned char keep[256];
    const int part = blockIdx.x, nparts = gridDim.x, s = blockIdx.y, tid = threadIdx.x;
    if (!emits(table, emit, s)) return;
    lh[tid] = 0u;
    keep[tid] = (unsigned char)kept_of(clock, trim, s, (unsigned)tid);
    __syncthreads();
    const KeptEvents pick{keep, nullptr};
    const float* const ps = pred + (long long)s * n;
    const PartRange r = part_range(part, chunk, n);
    unsigned acc = 0u, drop = 0u;
    for (int i = r.lo + 4 * tid; i < r.hi; i += TILE) {
        unsigned q[4], all;
        load_q4(ps, i, r.hi, vec, mc, q);
        all = sum_q4(q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                 // the rank needs the element's own n: before pick()
            const unsigned nq = q[k], kq = keep[nq];
            for (unsigned j = 0; j < kq; ++j) atomicAdd(&lh[gld<unsigned short>(rank + nq * 256u + j) & 255u], 1u);
        }
        pick(q, 0);
        acc += sum_q4(q);
        drop += all - sum_q4(q);
    }
    wave_fold_to(acc, Sum(), wsum);
    wave_fold_to(drop, Sum(), wdrop);
    __syncthreads();                                                  // (completes lh too)
    if (tid == 0) {
        gst<unsigned>(parts + (long long)s * nparts + part, lds_fold<NW>(wsum, Sum()));
        gst<unsigned>(dparts + (long long)s * nparts + part, lds_fold<NW>(wdrop, Sum()));
    }
    gst<unsigned>(hist + ((long long)s * hrows + part) * 256 + tid, lh[tid]);
}

// grid (nparts, S): emit_timed_expand_kernel on the kept events; part 0 also stores the slot's *dropped
__global__ __launch_bounds__(EMT) void emit_trimmed_expand_kernel(const bmc_slot_t* __restrict__ table,
                                                                  const bmc_slot_emit_timed_t* __restrict__ emit,
                                                                  const bmc_slot_clock_t* __restrict__ clock,
                                                                  const bmc_slot_trim_t* __restrict__ trim,
                                                                  const float* __restrict__ pred, int n, int chunk, int vec, float mc,
                                                                  const unsigned short* __restrict__ rank,
                                                                  const unsigned* __restrict__ dparts,
                                                                  const unsigned* __restrict__ hist, int hrows,
                                                                  const unsigned* __restrict__ dbase,
                                                                  const unsigned long long* __restrict__ tot, long long wcap,
                                                                  u32x2* __restrict__ rec) {
    __shared__ unsigned excl[TILE];          // exclusive prefix of keep[q] inside the tile
    __shared__ unsigned char qs[TILE];       // the tile's q
    __shared__ unsigned char keep[256];
    __shared__ unsigned wtot[NW];
    __shared__ unsigned long long red[NW];
    __shared__ unsigned run[256];
    __shared__ unsigned stepc[NW][256];
    const int part = blockIdx.x, nparts = gridDim.x, s = blockIdx.y, tid = threadIdx.x;
    if (!emits(table, emit, s)) return;
    if (part == 0) {                                                  // (uniform) a window that is not stored has lost events too
        const unsigned long long dropped = sum_parts<NW>(dparts + (long long)s * nparts, nparts, red);
        long long* const dst = gld<long long*>(&trim[s].dropped);
        if (tid == 0 && dst) gst<long long>(dst, (long long)dropped);
    }
    if (gld<unsigned long long>(tot + s) > (unsigned long long)wcap) return;
    keep[tid] = (unsigned char)kept_of(clock, trim, s, (unsigned)tid);
    run[tid] = gld<unsigned>(dbase + (long long)s * 256 + tid) + gld<unsigned>(hist + ((long long)s * hrows + part) * 256 + tid);
    stepc[0][tid] = stepc[1][tid] = stepc[2][tid] = stepc[3][tid] = 0u;
    __syncthreads();
    const KeptEvents pick{keep, qs};
    u32x2* const out = rec + (long long)s * wcap;
    const float* const ps = pred + (long long)s * n;
    const PartRange r = part_range(part, chunk, n);
    for (int tb = r.lo; tb < r.hi; tb += TILE) {                      // (uniform over the workgroup)
        const unsigned ttot = tile_scan(ps, tb, r.hi, vec, mc, excl, wtot, tid, pick);
        for (unsigned p0 = 0u; p0 < ttot; p0 += EMT) {                // 256 consecutive kept events of the tile per step
            const unsigned p = p0 + tid;
            const bool valid = p < ttot;
            unsigned key = 0u, idx = 0u;
            if (valid) {
                const int e = tile_owner(excl, p);
                const unsigned nq = qs[e], j = p - excl[e];           // the element's ORIGINAL n: rank and time depend on it
                idx = (unsigned)(tb + e);
                key = ((unsigned)gld<unsigned short>(rank + nq * 256u + j) << 16) | (j << 8) | nq;
            }
            const unsigned pos = place(run, stepc, valid, (key >> 16) & 255u, tid);
            if (valid && (long long)pos < wcap) gst<u32x2>(out + pos, u32x2{idx, key});
        }
    }
}

}  // namespace

extern "C" int bmc_slot_emit_trimmed(const bmc_slot_t* table, const bmc_slot_emit_timed_t* emit, const bmc_slot_clock_t* clock,
                                     const bmc_slot_trim_t* trim, int S, const float* pred, int sH, int sW, int max_count,
                                     int nparts, unsigned* parts, const unsigned short* rank_table, void* scratch,
                                     long long window_capacity, bmc_stream_t s) {
    BMC_CHECK_ARG(clock && ((unsigned long long)clock & 7ull) == 0,
                  "bmc_slot_emit_trimmed: the clock table must be an 8-byte aligned device array of S entries");
    BMC_CHECK_ARG(trim && ((unsigned long long)trim & 7ull) == 0,
                  "bmc_slot_emit_trimmed: the trim table must be an 8-byte aligned device array of S entries");
    EmitTimedPlan p;
    if (bmc_emit_timed_plan("bmc_slot_emit_trimmed", table, emit, clock, S, pred, sH, sW, max_count, nparts, parts, rank_table,
                            scratch, window_capacity, s, &p))
        return -1;
    unsigned* const dparts = parts + (long long)S * nparts;
    hipLaunchKernelGGL(emit_trimmed_count_kernel, dim3(nparts, S), dim3(EMT), 0, p.st, table, emit, clock, trim, pred, p.g.n,
                       p.g.chunk, p.g.vec, p.mc, rank_table, parts, dparts, p.hist, p.hrows);
    BMC_CHECK_LAUNCH("bmc_slot_emit_trimmed (count)");
    if (const int rc = bmc_emit_timed_scan_parts(p)) return rc;
    hipLaunchKernelGGL(emit_trimmed_expand_kernel, dim3(nparts, S), dim3(EMT), 0, p.st, table, emit, clock, trim, pred, p.g.n,
                       p.g.chunk, p.g.vec, p.mc, rank_table, (const unsigned*)dparts, (const unsigned*)p.hist, p.hrows,
                       (const unsigned*)p.dbase, (const unsigned long long*)p.tot, window_capacity, p.rec);
    BMC_CHECK_LAUNCH("bmc_slot_emit_trimmed (expand)");
    return bmc_emit_timed_high_pass(p);
}
