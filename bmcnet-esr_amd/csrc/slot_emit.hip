// Event output of multi-stream inference (bmcnet-esr_amd/infer.py::MultiStreamSR(emit_events=True)): per window and for all
// slots, the prediction [2][sH][sW] becomes an event list appended to the recording's own output columns (xs / ys int16, ps
// int8) -- the rounded, clamped count image that the reference renders (infer_BMCNet.py:94: esr_cnt[0].cpu().round()), as the
// stream whose encoding (slot_events.hip, flags 0) gives that image back exactly.
//   q = v > 0 ? min(rint(v), max_count) : 0  (round-half-to-even; NaN -> 0, +inf -> max_count);  element (c, row, x), visited
//   in the flat order of [2][sH][sW], contributes q consecutive events  xs = x, ys = sH-1-row, ps = c == 0 ? +1 : -1.
//
// An ordered stream compaction in TWO launches, grid (nparts, S), so that no workgroup ever waits for another one (no look-back,
// no flags, no atomics on global memory):
//   slot_emit_count_kernel   workgroup (part, s) sums q over its fixed contiguous chunk of slot s -> parts[s][part];
//   slot_emit_write_kernel   workgroup (part, s) adds the totals of the parts before it to *index_in (the recording's running
//                            event count), scans its chunk tile by tile (wave_k.h's block_scan_excl: a wave scan, one LDS exchange
//                            between the waves) and stores the events at their final positions; positions >= capacity are dropped.
//                            Workgroup 0 of the slot writes *index_out = *index_in + the slot's total: a different word from the
//                            one every workgroup reads, so there is no ordering requirement inside the launch.
// A tile's events are expanded position by position: lane p finds the element that owns output position p by a binary search in
// the tile's exclusive prefix (LDS), so consecutive lanes store consecutive events whatever the counts are (a pixel of 255
// events costs what 255 pixels of one event cost).  Counts are integers: the same bytes run after run.
// slot_emit_k.h holds what slot_emit_timed.hip shares: the quantisation, the tile scan, the search and the event's three stores.
#include "slot_emit_k.h"

namespace {

// grid (nparts, S): part p owns elements [p * chunk, min(n, (p+1) * chunk)) of the slot's n = 2*sH*sW
__global__ __launch_bounds__(EMT) void slot_emit_count_kernel(const bmc_slot_t* __restrict__ table,
                                                              const bmc_slot_emit_t* __restrict__ emit,
                                                              const float* __restrict__ pred, int n, int chunk, int vec, float mc,
                                                              unsigned* __restrict__ parts) {
    __shared__ unsigned wsum[NW];
    const int part = blockIdx.x, nparts = gridDim.x, s = blockIdx.y, tid = threadIdx.x;
    if (!emits(table, emit, s)) return;
    const float* const ps = pred + (long long)s * n;
    const PartRange r = part_range(part, chunk, n);
    unsigned acc = 0u;
    for (int i = r.lo + 4 * tid; i < r.hi; i += TILE) {
        unsigned q[4];
        load_q4(ps, i, r.hi, vec, mc, q);
        acc += sum_q4(q);
    }
    acc = block_fold<NW>(acc, Sum(), wsum);
    if (tid == 0) gst<unsigned>(parts + (long long)s * nparts + part, acc);
}

__global__ __launch_bounds__(EMT) void slot_emit_write_kernel(const bmc_slot_t* __restrict__ table,
                                                              const bmc_slot_emit_t* __restrict__ emit,
                                                              const float* __restrict__ pred, int sH, int sW, int n, int chunk,
                                                              int vec, float mc, const unsigned* __restrict__ parts) {
    __shared__ unsigned excl[TILE];          // exclusive prefix of q inside the tile
    __shared__ unsigned wtot[NW];
    __shared__ unsigned long long red[NW];
    const int part = blockIdx.x, nparts = gridDim.x, s = blockIdx.y, tid = threadIdx.x;
    if (!emits(table, emit, s)) return;
    const bmc_slot_emit_t* const ent = emit + s;
    short* const xs = gld<short*>(&ent->xs);
    short* const ys = gld<short*>(&ent->ys);
    signed char* const pol = gld<signed char*>(&ent->ps);
    const long long cap = gld<long long>(&ent->capacity);
    const long long base = gld<long long>(gld<const long long*>(&ent->index_in));
    // events of the parts before this one; workgroup 0 has none before it and adds ALL parts instead: the slot's total
    const unsigned* const pp = parts + (long long)s * nparts;
    const unsigned long long before = sum_parts<NW>(pp, part == 0 ? nparts : part, red);
    long long gpos = base + (long long)before;
    if (part == 0) {
        if (tid == 0) gst<long long>(gld<long long*>(&ent->index_out), gpos);
        gpos = base;
    }
    const float* const ps = pred + (long long)s * n;
    const PartRange r = part_range(part, chunk, n);
    const unsigned hw = (unsigned)sH * (unsigned)sW;
    for (int tb = r.lo; tb < r.hi; tb += TILE) {                      // (uniform over the workgroup)
        const unsigned ttot = tile_scan(ps, tb, r.hi, vec, mc, excl, wtot, tid);
        for (unsigned p = tid; p < ttot; p += EMT) {                  // output position p of the tile -> its element
            const long long pos = gpos + p;
            if (pos >= cap) break;                                    // (positions only grow with p)
            store_event(xs, ys, pol, pos, (unsigned)(tb + tile_owner(excl, p)), sH, sW, hw);
        }
        gpos += ttot;
    }
}

}  // namespace

extern "C" int bmc_slot_emit(const bmc_slot_t* table, const bmc_slot_emit_t* emit, int S, const float* pred, int sH, int sW,
                             int max_count, int nparts, unsigned* parts, bmc_stream_t s) {
    BMC_CHECK_ARG(max_count >= 1 && max_count <= 32767, "bmc_slot_emit: 1 <= max_count <= 32767 (got %d)", max_count);
    EmitGeom g;
    if (emit_geometry("bmc_slot_emit", table, emit, pred, parts, S, sH, sW, max_count, nparts, &g)) return -1;
    hipLaunchKernelGGL(slot_emit_count_kernel, dim3(nparts, S), dim3(EMT), 0, (hipStream_t)s, table, emit, pred, g.n, g.chunk,
                       g.vec, (float)max_count, parts);
    BMC_CHECK_LAUNCH("bmc_slot_emit (count)");
    hipLaunchKernelGGL(slot_emit_write_kernel, dim3(nparts, S), dim3(EMT), 0, (hipStream_t)s, table, emit, pred, sH, sW, g.n,
                       g.chunk, g.vec, (float)max_count, (const unsigned*)parts);
    BMC_CHECK_LAUNCH("bmc_slot_emit (write)");
    return 0;
}
