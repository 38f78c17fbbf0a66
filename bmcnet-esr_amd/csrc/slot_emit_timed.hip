// Timed event output of multi-stream inference (MultiStreamSR(emit_events=True, event_times="linear")): the events of
// slot_emit.hip, each with a float32 time inside its window, every window stored in time order (include/bmc_hip.h,
// bmc_slot_emit_timed).  Event j of an element with n = q events has the time t0 + (t1 - t0) * j / (n - 1) (t0 for n = 1) -- the
// reference's linear redistribution (dataloader/encodings.py:367-414) -- and the window is sorted by the EXACT rational
// j / (n - 1), equal rationals in flat emission order.  The sort key is the rational's dense rank among all fractions with
// denominators <= 254 (a host-built [256][256] uint16 table, rank_table[n][j]): fewer than 2^16 values, so a stable
// least-significant-digit radix sort in two 8-bit passes is exact.
//
// SIX launches per window for all slots; no workgroup waits for another, no atomics on global memory (histograms are
// counted with integer LDS atomics: order independent), every grid is fixed by the arguments:
//   count    (nparts, S)  part p of slot s sums q over its chunk -> parts[s][p], and counts the LOW digits of its events
//                         -> hist[s][p][256];
//   scan     (S)          the slot's total -> tot[s], *index_out = *index_in + total; the histograms become exclusive
//                         offsets over (digit, part); a window of more than window_capacity events stops here;
//   expand   (nparts, S)  part p walks its chunk tile by tile as slot_emit_write_kernel does and stores the record of every
//                         event (flat element index; rank, j, n) at its position by low digit in the slot's record buffer;
//   hist     (blocks, S)  block b counts the HIGH digits of records [b * T2, (b+1) * T2) of that buffer;
//   scan     (S)          ... exclusive offsets over (digit, block);
//   scatter  (blocks, S)  block b stores xs / ys / ps / ts of its records at *index_in + position by high digit; positions
//                         >= capacity are dropped.
// Stability: a workgroup handles its records 256 at a time in sequence order; the position of a record among those of its
// digit is (the workgroup's running count of the digit) + (the digit's counts of the lower waves in this step) + (the lanes
// below it in its wave with the same digit: eight ballots).
//
// Clocked output (bmc_slot_emit_clocked): the same six launches with a fourth table of bmc_slot_clock_t.  A slot whose clock
// entry has a `ts` column stores float64 times on the recording's own clock there instead of the float32 column:
// t = t_first + tau * (t_last - t_first), tau = T0 + (T1 - T0) * (j / g) / ((n - 1) / g), g = gcd(j, n - 1) -- the reduced
// fraction gives equal rationals ONE tau, so the float64 column cannot decrease inside a run of ties.  Only the scatter
// kernel reads the clock table; a NULL table (bmc_slot_emit_timed) or a NULL `ts` keeps the float32 behaviour.
//
// place() and clock_time() live in slot_emit_k.h: slot_emit_trimmed.hip (bmc_slot_emit_trimmed) splits and times its events
// with them, and launches this file's first scan, histogram, second scan and scatter kernel through bmc_emit_timed_plan /
// _scan_parts / _high_pass below.
#include "slot_emit_k.h"

namespace {

// grid (nparts, S): part p owns elements [p * chunk, min(n, (p+1) * chunk)) of the slot's n = 2*sH*sW
__global__ __launch_bounds__(EMT) void emit_timed_count_kernel(const bmc_slot_t* __restrict__ table,
                                                               const bmc_slot_emit_timed_t* __restrict__ emit,
                                                               const float* __restrict__ pred, int n, int chunk, int vec,
                                                               float mc, const unsigned short* __restrict__ rank,
                                                               unsigned* __restrict__ parts, unsigned* __restrict__ hist,
                                                               int hrows) {
    __shared__ unsigned wsum[NW];
    __shared__ unsigned lh[256];
    const int part = blockIdx.x, nparts = gridDim.x, s = blockIdx.y, tid = threadIdx.x;
    if (!emits(table, emit, s)) return;
    lh[tid] = 0u;
    __syncthreads();
    const float* const ps = pred + (long long)s * n;
    const PartRange r = part_range(part, chunk, n);
    unsigned acc = 0u;
    for (int i = r.lo + 4 * tid; i < r.hi; i += TILE) {
        unsigned q[4];
        load_q4(ps, i, r.hi, vec, mc, q);
        acc += sum_q4(q);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            for (unsigned j = 0; j < q[k]; ++j) atomicAdd(&lh[gld<unsigned short>(rank + q[k] * 256u + j) & 255u], 1u);
    }
    acc = block_fold<NW>(acc, Sum(), wsum);                           // (its barrier completes lh too)
    if (tid == 0) gst<unsigned>(parts + (long long)s * nparts + part, acc);
    gst<unsigned>(hist + ((long long)s * hrows + part) * 256 + tid, lh[tid]);
}

// grid (S).  first: rows = nparts histograms of the count pass; the slot's total and *index_out are written here.
// Otherwise rows = the blocks of the high-digit pass that hold records.  hist[s][row][d] -> the records of digit d in the rows
// before `row`; dbase[s][d] -> the records of the digits below d.
__global__ __launch_bounds__(EMT) void emit_timed_scan_kernel(const bmc_slot_t* __restrict__ table,
                                                              const bmc_slot_emit_timed_t* __restrict__ emit, int first,
                                                              int nparts, const unsigned* __restrict__ parts,
                                                              unsigned* __restrict__ hist, int hrows,
                                                              unsigned* __restrict__ dbase, unsigned long long* __restrict__ tot,
                                                              long long wcap) {
    __shared__ unsigned long long red[NW];
    __shared__ unsigned wtot[NW];
    const int s = blockIdx.x, tid = threadIdx.x;
    if (!emits(table, emit, s)) return;
    unsigned long long total;
    if (first) {
        total = sum_parts<NW>(parts + (long long)s * nparts, nparts, red);
        if (tid == 0) {
            const bmc_slot_emit_timed_t* const ent = emit + s;
            gst<unsigned long long>(tot + s, total);
            gst<long long>(gld<long long*>(&ent->index_out),
                           gld<long long>(gld<const long long*>(&ent->index_in)) + (long long)total);
        }
    } else {
        total = gld<unsigned long long>(tot + s);
    }
    if (total > (unsigned long long)wcap) return;                     // (uniform) the window does not fit: nothing is sorted
    const int rows = first ? nparts : (int)((total + T2 - 1) / T2);
    unsigned* const h = hist + (long long)s * hrows * 256 + tid;      // thread t owns digit t
    unsigned running = 0u;
    for (int r0 = 0; r0 < rows; r0 += 8) {
        unsigned v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = r0 + k < rows ? gld<unsigned>(h + (long long)(r0 + k) * 256) : 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (r0 + k < rows) gst<unsigned>(h + (long long)(r0 + k) * 256, running);
            running += v[k];
        }
    }
    unsigned all;                                                     // exclusive scan of the digit totals over the workgroup
    gst<unsigned>(dbase + (long long)s * 256 + tid, block_scan_excl<NW>(running, wtot, &all));
}

// grid (nparts, S): the events of part p, in flat order, to their positions by low digit in rec[s]
__global__ __launch_bounds__(EMT) void emit_timed_expand_kernel(const bmc_slot_t* __restrict__ table,
                                                                const bmc_slot_emit_timed_t* __restrict__ emit,
                                                                const float* __restrict__ pred, int n, int chunk, int vec,
                                                                float mc, const unsigned short* __restrict__ rank,
                                                                const unsigned* __restrict__ hist, int hrows,
                                                                const unsigned* __restrict__ dbase,
                                                                const unsigned long long* __restrict__ tot, long long wcap,
                                                                u32x2* __restrict__ rec) {
    __shared__ unsigned excl[TILE];          // exclusive prefix of q inside the tile
    __shared__ unsigned wtot[NW];
    __shared__ unsigned run[256];
    __shared__ unsigned stepc[NW][256];
    const int part = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    if (!emits(table, emit, s)) return;
    if (gld<unsigned long long>(tot + s) > (unsigned long long)wcap) return;
    run[tid] = gld<unsigned>(dbase + (long long)s * 256 + tid) + gld<unsigned>(hist + ((long long)s * hrows + part) * 256 + tid);
    stepc[0][tid] = stepc[1][tid] = stepc[2][tid] = stepc[3][tid] = 0u;
    u32x2* const out = rec + (long long)s * wcap;
    const float* const ps = pred + (long long)s * n;
    const PartRange r = part_range(part, chunk, n);
    for (int tb = r.lo; tb < r.hi; tb += TILE) {                      // (uniform over the workgroup)
        const unsigned ttot = tile_scan(ps, tb, r.hi, vec, mc, excl, wtot, tid);
        for (unsigned p0 = 0u; p0 < ttot; p0 += EMT) {                // 256 consecutive events of the tile per step
            const unsigned p = p0 + tid;
            const bool valid = p < ttot;
            unsigned key = 0u, idx = 0u;
            if (valid) {
                const int e = tile_owner(excl, p);
                const unsigned first = excl[e], nq = (e + 1 < TILE ? excl[e + 1] : ttot) - first, j = p - first;
                idx = (unsigned)(tb + e);
                key = ((unsigned)gld<unsigned short>(rank + nq * 256u + j) << 16) | (j << 8) | nq;
            }
            const unsigned pos = place(run, stepc, valid, (key >> 16) & 255u, tid);
            if (valid && (long long)pos < wcap) gst<u32x2>(out + pos, u32x2{idx, key});
        }
    }
}

// grid (blocks, S): the high digits of records [b * T2, min(total, (b+1) * T2)) of rec[s] -> hist[s][b][256]
__global__ __launch_bounds__(EMT) void emit_timed_hist_kernel(const bmc_slot_t* __restrict__ table,
                                                              const bmc_slot_emit_timed_t* __restrict__ emit,
                                                              unsigned* __restrict__ hist, int hrows,
                                                              const unsigned long long* __restrict__ tot, long long wcap,
                                                              const u32x2* __restrict__ rec) {
    __shared__ unsigned lh[256];
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    if (!emits(table, emit, s)) return;
    const unsigned long long total = gld<unsigned long long>(tot + s);
    const long long lo = (long long)b * T2;
    if (total > (unsigned long long)wcap || lo >= (long long)total) return;
    const long long hi = lo + T2 < (long long)total ? lo + T2 : (long long)total;
    lh[tid] = 0u;
    __syncthreads();
    const u32x2* const in = rec + (long long)s * wcap;
    for (long long i = lo + tid; i < hi; i += EMT) atomicAdd(&lh[gld<u32x2>(in + i).y >> 24], 1u);
    __syncthreads();
    gst<unsigned>(hist + ((long long)s * hrows + b) * 256 + tid, lh[tid]);
}

// grid (blocks, S): records [b * T2, ...) of rec[s], in their order, to the columns at *index_in + position by high digit.
// clock: NULL, or the table of bmc_slot_emit_clocked; a slot with clock[s].ts stores float64 clock times there, not ts.
__global__ __launch_bounds__(EMT) void emit_timed_scatter_kernel(const bmc_slot_t* __restrict__ table,
                                                                 const bmc_slot_emit_timed_t* __restrict__ emit,
                                                                 const bmc_slot_clock_t* __restrict__ clock, int sH, int sW,
                                                                 const unsigned* __restrict__ hist, int hrows,
                                                                 const unsigned* __restrict__ dbase,
                                                                 const unsigned long long* __restrict__ tot, long long wcap,
                                                                 const u32x2* __restrict__ rec) {
    __shared__ unsigned run[256];
    __shared__ unsigned stepc[NW][256];
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    if (!emits(table, emit, s)) return;
    const unsigned long long total = gld<unsigned long long>(tot + s);
    const long long lo = (long long)b * T2;
    if (total > (unsigned long long)wcap || lo >= (long long)total) return;
    const long long hi = lo + T2 < (long long)total ? lo + T2 : (long long)total;
    const bmc_slot_emit_timed_t* const ent = emit + s;
    short* const xs = gld<short*>(&ent->xs);
    short* const ys = gld<short*>(&ent->ys);
    signed char* const pol = gld<signed char*>(&ent->ps);
    float* const ts = gld<float*>(&ent->ts);
    const long long cap = gld<long long>(&ent->capacity);
    const long long base = gld<long long>(gld<const long long*>(&ent->index_in));
    double* const ts64 = clock ? gld<double*>(&clock[s].ts) : nullptr;                    // (uniform) the slot is clocked
    const double t_first = ts64 ? gld<double>(&clock[s].t_first) : 0.0;
    const double dt = ts64 ? gld<double>(&clock[s].t_last) - t_first : 0.0;
    run[tid] = gld<unsigned>(dbase + (long long)s * 256 + tid) + gld<unsigned>(hist + ((long long)s * hrows + b) * 256 + tid);
    stepc[0][tid] = stepc[1][tid] = stepc[2][tid] = stepc[3][tid] = 0u;
    __syncthreads();
    const u32x2* const in = rec + (long long)s * wcap;
    const unsigned hw = (unsigned)sH * (unsigned)sW;
    for (long long i0 = lo; i0 < hi; i0 += EMT) {                     // (uniform over the workgroup)
        const long long i = i0 + tid;
        const bool valid = i < hi;
        u32x2 r = u32x2{0u, 0u};
        if (valid) r = gld<u32x2>(in + i);
        const long long pos = base + place(run, stepc, valid, r.y >> 24, tid);
        if (valid && pos < cap) {
            const unsigned idx = r.x, j = (r.y >> 8) & 255u, nq = r.y & 255u;
            store_event(xs, ys, pol, pos, idx, sH, sW, hw);
            if (ts64) {
                gst<double>(ts64 + pos, clock_time(t_first, dt, j, nq));
            } else {
                // float64, rounded once: t0 + (t1 - t0) * j / (n - 1)
                const double t = nq > 1u ? BMC_EVENT_T0 + (BMC_EVENT_T1 - BMC_EVENT_T0) * (double)j / (double)(nq - 1u) : BMC_EVENT_T0;
                gst<float>(ts + pos, (float)t);
            }
        }
    }
}

long long hist_rows(int nparts, long long wcap) {
    const long long blocks = (wcap + T2 - 1) / T2;
    return blocks > nparts ? blocks : nparts;
}

}  // namespace

extern "C" long long bmc_slot_emit_timed_scratch_bytes(int S, int nparts, long long window_capacity) {
    if (S < 1 || S > BMC_MAX_SLOTS || nparts < 1 || nparts > BMC_SLOT_EMIT_MAX_PARTS || window_capacity < 1 ||
        window_capacity > BMC_SLOT_EMIT_TIMED_MAX_WINDOW)
        return -1;
    // records [S][window_capacity] x 8, totals [S] x 8, digit bases [S][256] x 4, histograms [S][rows][256] x 4
    return (long long)S * (8 * window_capacity + 8 + 1024 + 1024 * hist_rows(nparts, window_capacity));
}

int bmc_emit_timed_plan(const char* who, const bmc_slot_t* table, const bmc_slot_emit_timed_t* emit, const bmc_slot_clock_t* clock,
                        int S, const float* pred, int sH, int sW, int max_count, int nparts, unsigned* parts,
                        const unsigned short* rank_table, void* scratch, long long window_capacity, bmc_stream_t s,
                        EmitTimedPlan* p) {
    BMC_CHECK_ARG(rank_table && scratch, "%s: bad arguments", who);
    BMC_CHECK_ARG(max_count >= 1 && max_count <= BMC_SLOT_EMIT_TIMED_MAX_COUNT,
                  "%s: 1 <= max_count <= %d (the rank table; got %d)", who, BMC_SLOT_EMIT_TIMED_MAX_COUNT, max_count);
    BMC_CHECK_ARG(window_capacity >= 1 && window_capacity <= BMC_SLOT_EMIT_TIMED_MAX_WINDOW,
                  "%s: 1 <= window_capacity <= %lld (got %lld)", who, (long long)BMC_SLOT_EMIT_TIMED_MAX_WINDOW,
                  window_capacity);
    BMC_CHECK_ARG(((unsigned long long)pred & 3ull) == 0 && ((unsigned long long)scratch & 7ull) == 0 &&
                      ((unsigned long long)rank_table & 1ull) == 0,
                  "%s: pred must be 4-byte, scratch 8-byte, rank_table 2-byte aligned", who);
    if (emit_geometry(who, table, emit, pred, parts, S, sH, sW, max_count, nparts, &p->g)) return -1;
    p->table = table, p->emit = emit, p->clock = clock, p->S = S, p->sH = sH, p->sW = sW, p->nparts = nparts;
    p->blocks = (int)((window_capacity + T2 - 1) / T2), p->hrows = (int)hist_rows(nparts, window_capacity);
    p->mc = (float)max_count, p->pred = pred, p->parts = parts, p->rank = rank_table, p->wcap = window_capacity;
    p->rec = (u32x2*)scratch;
    p->tot = (unsigned long long*)(p->rec + (long long)S * window_capacity);
    p->dbase = (unsigned*)(p->tot + S);
    p->hist = p->dbase + (long long)S * 256;
    p->st = (hipStream_t)s;
    return 0;
}

int bmc_emit_timed_scan_parts(const EmitTimedPlan& p) {
    hipLaunchKernelGGL(emit_timed_scan_kernel, dim3(p.S), dim3(EMT), 0, p.st, p.table, p.emit, 1, p.nparts, (const unsigned*)p.parts,
                       p.hist, p.hrows, p.dbase, p.tot, p.wcap);
    BMC_CHECK_LAUNCH("bmc_slot_emit_timed (scan 1)");
    return 0;
}

int bmc_emit_timed_high_pass(const EmitTimedPlan& p) {
    hipLaunchKernelGGL(emit_timed_hist_kernel, dim3(p.blocks, p.S), dim3(EMT), 0, p.st, p.table, p.emit, p.hist, p.hrows,
                       (const unsigned long long*)p.tot, p.wcap, (const u32x2*)p.rec);
    BMC_CHECK_LAUNCH("bmc_slot_emit_timed (histogram)");
    hipLaunchKernelGGL(emit_timed_scan_kernel, dim3(p.S), dim3(EMT), 0, p.st, p.table, p.emit, 0, p.nparts, (const unsigned*)p.parts,
                       p.hist, p.hrows, p.dbase, p.tot, p.wcap);
    BMC_CHECK_LAUNCH("bmc_slot_emit_timed (scan 2)");
    hipLaunchKernelGGL(emit_timed_scatter_kernel, dim3(p.blocks, p.S), dim3(EMT), 0, p.st, p.table, p.emit, p.clock, p.sH, p.sW,
                       (const unsigned*)p.hist, p.hrows, (const unsigned*)p.dbase, (const unsigned long long*)p.tot, p.wcap,
                       (const u32x2*)p.rec);
    BMC_CHECK_LAUNCH("bmc_slot_emit_timed (scatter)");
    return 0;
}

namespace {

// the six launches of bmc_slot_emit_timed (clock == NULL) and bmc_slot_emit_clocked; `who` names the entry point in messages
int emit_timed_launch(const char* who, const bmc_slot_t* table, const bmc_slot_emit_timed_t* emit, const bmc_slot_clock_t* clock,
                      int S, const float* pred, int sH, int sW, int max_count, int nparts, unsigned* parts,
                      const unsigned short* rank_table, void* scratch, long long window_capacity, bmc_stream_t s) {
    EmitTimedPlan p;
    if (bmc_emit_timed_plan(who, table, emit, clock, S, pred, sH, sW, max_count, nparts, parts, rank_table, scratch, window_capacity,
                            s, &p))
        return -1;
    hipLaunchKernelGGL(emit_timed_count_kernel, dim3(nparts, S), dim3(EMT), 0, p.st, table, emit, pred, p.g.n, p.g.chunk, p.g.vec,
                       p.mc, rank_table, parts, p.hist, p.hrows);
    BMC_CHECK_LAUNCH("bmc_slot_emit_timed (count)");
    if (const int rc = bmc_emit_timed_scan_parts(p)) return rc;
    hipLaunchKernelGGL(emit_timed_expand_kernel, dim3(nparts, S), dim3(EMT), 0, p.st, table, emit, pred, p.g.n, p.g.chunk, p.g.vec,
                       p.mc, rank_table, (const unsigned*)p.hist, p.hrows, (const unsigned*)p.dbase,
                       (const unsigned long long*)p.tot, window_capacity, p.rec);
    BMC_CHECK_LAUNCH("bmc_slot_emit_timed (expand)");
    return bmc_emit_timed_high_pass(p);
}

}  // namespace

extern "C" int bmc_slot_emit_timed(const bmc_slot_t* table, const bmc_slot_emit_timed_t* emit, int S, const float* pred, int sH,
                                   int sW, int max_count, int nparts, unsigned* parts, const unsigned short* rank_table,
                                   void* scratch, long long window_capacity, bmc_stream_t s) {
    return emit_timed_launch("bmc_slot_emit_timed", table, emit, nullptr, S, pred, sH, sW, max_count, nparts, parts, rank_table,
                             scratch, window_capacity, s);
}

extern "C" int bmc_slot_emit_clocked(const bmc_slot_t* table, const bmc_slot_emit_timed_t* emit, const bmc_slot_clock_t* clock,
                                     int S, const float* pred, int sH, int sW, int max_count, int nparts, unsigned* parts,
                                     const unsigned short* rank_table, void* scratch, long long window_capacity, bmc_stream_t s) {
    BMC_CHECK_ARG(clock && ((unsigned long long)clock & 7ull) == 0,
                  "bmc_slot_emit_clocked: the clock table must be an 8-byte aligned device array of S entries");
    return emit_timed_launch("bmc_slot_emit_clocked", table, emit, clock, S, pred, sH, sW, max_count, nparts, parts, rank_table,
                             scratch, window_capacity, s);
}
