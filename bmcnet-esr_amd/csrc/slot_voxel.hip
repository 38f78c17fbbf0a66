// Voxel grids of the slots' predictions (MultiStreamSR(voxel_bins=B)): the contract is in include/bmc_hip.h ("voxel grids").
// bmc_slot_voxel gives, per slot with a voxel entry, the [bins][sH][sW] grid the reference's events_to_voxel_torch
// (dataloader/encodings.py:100-148, temporal_bilinear=True) returns for the slot's TIMED event stream (bmc_slot_emit_timed) --
// without building that stream.  In a timed window event j of an element with n events has a time that depends on (j, n) only,
// the events of output pixel (y, x) are those of the two elements P[0][sH-1-y][x] and P[1][sH-1-y][x], and the reference's
// normalisation needs two facts about the whole window: whether it has more than 3 events, and whether any element has 2 or
// more (then the last time is 1.0, else every time is 0.01).  So a pixel's `bins` values are a closed form of its two counts:
// its two runs merged in the stream's order (the exact rational j / (n - 1), channel 0 first on ties) and accumulated in
// float32 exactly as the reference's index_put_(accumulate=True) adds them, bin by bin.
//
// TWO launches for all slots; no memset, no atomics, no workgroup waits for another:
//   reduce  (nparts, S)  part p of slot s sums q over its chunk of the 2*sH*sW elements and takes the largest q
//                        -> parts[s][0][p], parts[s][1][p];
//   voxel   (nparts, S)  every workgroup folds its slot's nparts partials (in part order, as sum_parts does), then lane by lane
//                        owns output pixels of its chunk of the sH*sW pixels: two loads, `bins` stores, both coalesced along x
//                        (the flipped row is still a contiguous row).
// The per-pixel loop is data dependent (counts differ between lanes); predictions are sparse, so the launch is bound by its
// 4 * bins * sH * sW bytes of stores per slot.
#include "slot_emit_k.h"

namespace {

// the slot has a grid this window: it is active, has a prediction and its voxel entry has a dst (uniform over the workgroup)
__device__ __forceinline__ bool voxels(const bmc_slot_t* table, const bmc_slot_voxel_t* voxel, int s) {
    return (gld<int>(&table[s].flags) & BMC_SLOT_ACTIVE) && gld<const float*>(&table[s].frames) != nullptr &&
           gld<float*>(&voxel[s].dst) != nullptr;
}

// grid (nparts, S): part p owns elements [p * chunk, min(n, (p+1) * chunk)) of the slot's n = 2*sH*sW
__global__ __launch_bounds__(EMT) void slot_voxel_reduce_kernel(const bmc_slot_t* __restrict__ table,
                                                                const bmc_slot_voxel_t* __restrict__ voxel,
                                                                const float* __restrict__ pred, int n, int chunk, int vec,
                                                                float mc, unsigned* __restrict__ parts) {
    __shared__ unsigned wsum[NW], wmax[NW];
    const int part = blockIdx.x, nparts = gridDim.x, s = blockIdx.y, tid = threadIdx.x;
    if (!voxels(table, voxel, s)) return;
    const float* const ps = pred + (long long)s * n;
    const PartRange r = part_range(part, chunk, n);
    unsigned acc = 0u, big = 0u;
    for (int i = r.lo + 4 * tid; i < r.hi; i += TILE) {
        unsigned q[4];
        load_q4(ps, i, r.hi, vec, mc, q);
        acc += sum_q4(q);
        const unsigned a = q[0] > q[1] ? q[0] : q[1], b = q[2] > q[3] ? q[2] : q[3], m = a > b ? a : b;
        big = big > m ? big : m;
    }
    acc = block_fold<NW>(acc, Sum(), wsum);
    big = block_fold<NW>(big, Max(), wmax);
    if (tid == 0) {
        unsigned* const pp = parts + 2ll * s * nparts + part;
        gst<unsigned>(pp, acc);
        gst<unsigned>(pp + nparts, big);
    }
}

// float32 time of event j of an element's n events: the timed contract's expression (float64, rounded once), as
// emit_timed_scatter_kernel evaluates it
__device__ __forceinline__ float event_time(unsigned j, unsigned nq) {
    const double t = nq > 1u ? BMC_EVENT_T0 + (BMC_EVENT_T1 - BMC_EVENT_T0) * (double)j / (double)(nq - 1u) : BMC_EVENT_T0;
    return (float)t;
}

// grid (nparts, S): part p owns output pixels [p * pchunk, min(hw, (p+1) * pchunk)) of the slot's hw = sH*sW
__global__ __launch_bounds__(EMT) void slot_voxel_kernel(const bmc_slot_t* __restrict__ table,
                                                         const bmc_slot_voxel_t* __restrict__ voxel,
                                                         const float* __restrict__ pred, int sH, int sW, int pchunk, float mc,
                                                         int bins, const unsigned* __restrict__ parts) {
#pragma clang fp contract(off)      // every float32 operation is rounded on its own, as the reference's tensor expressions are
    __shared__ unsigned long long red[NW];
    __shared__ unsigned wmax[NW];
    const int part = blockIdx.x, nparts = gridDim.x, s = blockIdx.y, tid = threadIdx.x;
    if (!voxels(table, voxel, s)) return;
    const int hw = sH * sW;
    const unsigned* const pp = parts + 2ll * s * nparts;
    unsigned big = 0u;
    for (int j = tid; j < nparts; j += EMT) {
        const unsigned v = gld<unsigned>(pp + nparts + j);
        big = big > v ? big : v;
    }
    big = block_fold_all<NW>(big, Max(), wmax);
    const unsigned long long total = sum_parts<NW>(pp, nparts, red);
    const bool live = total > 3ull;                                   // events_to_voxel_torch :122: len(ts) <= 3 -> zeros
    const float t_first = (float)BMC_EVENT_T0;
    const float t_last = big >= 2u ? (float)BMC_EVENT_T1 : (float)BMC_EVENT_T0;
    const float dt = (t_last - t_first) + 1e-6f;
    const float bm1 = (float)(bins - 1);
    const float* const p0 = pred + 2ll * s * hw;
    float* const dst = gld<float*>(&voxel[s].dst);
    const PartRange r = part_range(part, pchunk, hw);
    for (int o = r.lo + tid; o < r.hi; o += EMT) {
        float acc[BMC_SLOT_VOXEL_MAX_BINS];
#pragma unroll
        for (int bi = 0; bi < BMC_SLOT_VOXEL_MAX_BINS; ++bi) acc[bi] = 0.f;
        if (live) {
            const int y = o / sW, x = o - y * sW;
            const int src = (sH - 1 - y) * sW + x;                    // the output's rows are the sensor's y: the prediction's, flipped
            const unsigned q0 = quant(gld<float>(p0 + src), mc), q1 = quant(gld<float>(p0 + hw + src), mc);
            const unsigned d0 = q0 > 1u ? q0 - 1u : 1u, d1 = q1 > 1u ? q1 - 1u : 1u;
            unsigned i0 = 0u, i1 = 0u;
            while (i0 < q0 || i1 < q1) {                              // the two runs, merged by j / (n - 1); ties: channel 0 first
                const bool take0 = i1 >= q1 || (i0 < q0 && i0 * d1 <= i1 * d0);
                const float t = take0 ? event_time(i0, q0) : event_time(i1, q1);
                const float p = take0 ? 1.f : -1.f;
                i0 += take0 ? 1u : 0u;
                i1 += take0 ? 0u : 1u;
                const float tn = ((t - t_first) / dt) * bm1;
#pragma unroll
                for (int bi = 0; bi < BMC_SLOT_VOXEL_MAX_BINS; ++bi)
                    if (bi < bins) {
                        const float w = fmaxf(0.f, 1.0f - fabsf(tn - (float)bi));
                        acc[bi] = acc[bi] + p * w;
                    }
            }
        }
#pragma unroll
        for (int bi = 0; bi < BMC_SLOT_VOXEL_MAX_BINS; ++bi)
            if (bi < bins) gst<float>(dst + (long long)bi * hw + o, acc[bi]);
    }
}

}  // namespace

extern "C" int bmc_slot_voxel(const bmc_slot_t* table, const bmc_slot_voxel_t* voxel, int S, const float* pred, int sH, int sW,
                              int max_count, int bins, int nparts, unsigned* parts, bmc_stream_t s) {
    static_assert(sizeof(bmc_slot_voxel_t) == 8, "bmc_slot_voxel_t is one pointer");
    BMC_CHECK_ARG(max_count >= 1 && max_count <= BMC_SLOT_EMIT_TIMED_MAX_COUNT,
                  "bmc_slot_voxel: 1 <= max_count <= %d (the times are defined for n <= 255; got %d)",
                  BMC_SLOT_EMIT_TIMED_MAX_COUNT, max_count);
    BMC_CHECK_ARG(bins >= 1 && bins <= BMC_SLOT_VOXEL_MAX_BINS, "bmc_slot_voxel: 1 <= bins <= %d (got %d)",
                  BMC_SLOT_VOXEL_MAX_BINS, bins);
    EmitGeom g;
    if (emit_geometry("bmc_slot_voxel", table, voxel, pred, parts, S, sH, sW, max_count, nparts, &g)) return -1;
    BMC_CHECK_ARG(((unsigned long long)voxel & 7ull) == 0 && ((unsigned long long)parts & 3ull) == 0,
                  "bmc_slot_voxel: the voxel table must be 8-byte, parts 4-byte aligned");
    const int hw = sH * sW, pchunk = (hw + nparts - 1) / nparts;
    const hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(slot_voxel_reduce_kernel, dim3(nparts, S), dim3(EMT), 0, st, table, voxel, pred, g.n, g.chunk, g.vec,
                       (float)max_count, parts);
    BMC_CHECK_LAUNCH("bmc_slot_voxel (reduce)");
    hipLaunchKernelGGL(slot_voxel_kernel, dim3(nparts, S), dim3(EMT), 0, st, table, voxel, pred, sH, sW, pchunk, (float)max_count,
                       bins, (const unsigned*)parts);
    BMC_CHECK_LAUNCH("bmc_slot_voxel");
    return 0;
}
