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
//                            event count), scans its chunk tile by tile (wave scan with cross-lane moves, one LDS exchange between
//                            the waves) and stores the events at their final positions; positions >= capacity are dropped.
//                            Workgroup 0 of the slot writes *index_out = *index_in + the slot's total: a different word from the
//                            one every workgroup reads, so there is no ordering requirement inside the launch.
// A tile's events are expanded position by position: lane p finds the element that owns output position p by a binary search in
// the tile's exclusive prefix (LDS), so consecutive lanes store consecutive events whatever the counts are (a pixel of 255
// events costs what 255 pixels of one event cost).  Counts are integers: the same bytes run after run.
// Pointers read from the tables go through address-space(1) casts (global_* instructions, never flat_*), as in slots.hip.
#include "bmc_common.h"

namespace {

template <class T>
__device__ __forceinline__ T gld(const void* p) {
    return *(const __attribute__((address_space(1))) T*)(unsigned long long)p;
}
template <class T>
__device__ __forceinline__ void gst(void* p, T v) {
    *(__attribute__((address_space(1))) T*)(unsigned long long)p = v;
}

constexpr int EMT = 256;             // threads per workgroup (4 waves)
constexpr int NW = EMT / 64;
constexpr int TILE = 4 * EMT;        // elements per tile: 4 consecutive ones per lane

__device__ __forceinline__ unsigned quant(float v, float mc) { return v > 0.f ? (unsigned)fminf(rintf(v), mc) : 0u; }

// q of the 4 elements i .. i+3 of a slot's prediction, 0 beyond `hi`.  vec: i, hi and the slot's base are multiples of 4
__device__ __forceinline__ void load_q4(const float* ps, int i, int hi, bool vec, float mc, unsigned (&q)[4]) {
    q[0] = q[1] = q[2] = q[3] = 0u;
    if (i >= hi) return;
    if (vec) {
        const f32x4 v = gld<f32x4>(ps + i);
        q[0] = quant(v.x, mc); q[1] = quant(v.y, mc); q[2] = quant(v.z, mc); q[3] = quant(v.w, mc);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < hi) q[k] = quant(gld<float>(ps + i + k), mc);
    }
}

// the slot emits this window: it is active and its emit entry has columns (uniform over the workgroup)
__device__ __forceinline__ bool emits(const bmc_slot_t* table, const bmc_slot_emit_t* emit, int s) {
    return (gld<int>(&table[s].flags) & BMC_SLOT_ACTIVE) && gld<const float*>(&table[s].frames) != nullptr &&
           gld<short*>(&emit[s].xs) != nullptr;
}

// grid (nparts, S): part p owns elements [p * chunk, min(n, (p+1) * chunk)) of the slot's n = 2*sH*sW
__global__ __launch_bounds__(EMT) void slot_emit_count_kernel(const bmc_slot_t* __restrict__ table,
                                                              const bmc_slot_emit_t* __restrict__ emit,
                                                              const float* __restrict__ pred, int n, int chunk, int vec, float mc,
                                                              unsigned* __restrict__ parts) {
    __shared__ unsigned wsum[NW];
    const int part = blockIdx.x, nparts = gridDim.x, s = blockIdx.y, tid = threadIdx.x;
    if (!emits(table, emit, s)) return;
    const float* const ps = pred + (long long)s * n;
    const long long lo64 = (long long)part * chunk;
    const int lo = (int)(lo64 < n ? lo64 : n), hi = (int)(lo64 + chunk < n ? lo64 + chunk : n);
    unsigned acc = 0u;
    for (int i = lo + 4 * tid; i < hi; i += TILE) {
        unsigned q[4];
        load_q4(ps, i, hi, vec, mc, q);
        acc += q[0] + q[1] + q[2] + q[3];
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) gst<unsigned>(parts + (long long)s * nparts + part, wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(EMT) void slot_emit_write_kernel(const bmc_slot_t* __restrict__ table,
                                                              const bmc_slot_emit_t* __restrict__ emit,
                                                              const float* __restrict__ pred, int sH, int sW, int n, int chunk,
                                                              int vec, float mc, const unsigned* __restrict__ parts) {
    __shared__ unsigned excl[TILE];          // exclusive prefix of q inside the tile
    __shared__ unsigned wtot[NW];
    __shared__ unsigned long long red[NW];
    const int part = blockIdx.x, nparts = gridDim.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!emits(table, emit, s)) return;
    const bmc_slot_emit_t* const ent = emit + s;
    short* const xs = gld<short*>(&ent->xs);
    short* const ys = gld<short*>(&ent->ys);
    signed char* const pol = gld<signed char*>(&ent->ps);
    const long long cap = gld<long long>(&ent->capacity);
    const long long base = gld<long long>(gld<const long long*>(&ent->index_in));
    // events of the parts before this one; workgroup 0 has none before it and adds ALL parts instead: the slot's total
    const unsigned* const pp = parts + (long long)s * nparts;
    const int lim = part == 0 ? nparts : part;
    unsigned long long before = 0ull;
    for (int j = tid; j < lim; j += EMT) before += gld<unsigned>(pp + j);
    for (int o = 32; o > 0; o >>= 1) before += __shfl_down(before, o);
    if (lane == 0) red[wave] = before;
    __syncthreads();
    before = red[0] + red[1] + red[2] + red[3];
    long long gpos = base + (long long)before;
    if (part == 0) {
        if (tid == 0) gst<long long>(gld<long long*>(&ent->index_out), gpos);
        gpos = base;
    }
    const float* const ps = pred + (long long)s * n;
    const long long lo64 = (long long)part * chunk;
    const int lo = (int)(lo64 < n ? lo64 : n), hi = (int)(lo64 + chunk < n ? lo64 + chunk : n);
    const unsigned hw = (unsigned)sH * (unsigned)sW;
    for (int tb = lo; tb < hi; tb += TILE) {                          // (uniform over the workgroup)
        unsigned q[4];
        load_q4(ps, tb + 4 * tid, hi, vec, mc, q);
        const unsigned t = q[0] + q[1] + q[2] + q[3];
        unsigned inc = t;                                             // inclusive scan over the wave
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        unsigned woff = 0u, ttot = 0u;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const unsigned v = wtot[w];
            if (w < wave) woff += v;
            ttot += v;
        }
        const unsigned e0 = woff + inc - t;
        excl[4 * tid] = e0;
        excl[4 * tid + 1] = e0 + q[0];
        excl[4 * tid + 2] = e0 + q[0] + q[1];
        excl[4 * tid + 3] = e0 + q[0] + q[1] + q[2];
        __syncthreads();
        for (unsigned p = tid; p < ttot; p += EMT) {                  // output position p of the tile -> its element
            const long long pos = gpos + p;
            if (pos >= cap) break;                                    // (positions only grow with p)
            int e = 0;                                                // the largest e with excl[e] <= p: its q is > 0
#pragma unroll
            for (int step = TILE / 2; step > 0; step >>= 1)
                if (excl[e + step] <= p) e += step;
            const unsigned idx = (unsigned)(tb + e);
            const unsigned c = idx >= hw ? 1u : 0u, rem = idx - c * hw, row = rem / (unsigned)sW, x = rem - row * (unsigned)sW;
            gst<short>(xs + pos, (short)x);
            gst<short>(ys + pos, (short)(sH - 1 - (int)row));
            gst<signed char>(pol + pos, (signed char)(c ? -1 : 1));
        }
        gpos += ttot;
    }
}

}  // namespace

extern "C" int bmc_slot_emit(const bmc_slot_t* table, const bmc_slot_emit_t* emit, int S, const float* pred, int sH, int sW,
                             int max_count, int nparts, unsigned* parts, bmc_stream_t s) {
    BMC_CHECK_ARG(table && emit && pred && parts && S >= 1 && S <= BMC_MAX_SLOTS, "bmc_slot_emit: bad arguments");
    BMC_CHECK_ARG(sH >= 1 && sW >= 1 && sH <= 32767 && sW <= 32767,
                  "bmc_slot_emit: sH, sW must be 1 .. 32767 (coordinates are int16; got %d x %d)", sH, sW);
    BMC_CHECK_ARG(max_count >= 1 && max_count <= 32767, "bmc_slot_emit: 1 <= max_count <= 32767 (got %d)", max_count);
    BMC_CHECK_ARG(nparts >= 1 && nparts <= BMC_SLOT_EMIT_MAX_PARTS, "bmc_slot_emit: 1 <= nparts <= %d (got %d)",
                  BMC_SLOT_EMIT_MAX_PARTS, nparts);
    BMC_CHECK_ARG(((unsigned long long)pred & 3ull) == 0, "bmc_slot_emit: pred must be 4-byte aligned");
    const long long n = 2ll * sH * sW;                                // < 2^31 for sH, sW <= 32767
    const long long chunk = ((n + nparts - 1) / nparts + 3) / 4 * 4;
    BMC_CHECK_ARG(chunk * max_count < (1ll << 32),
                  "bmc_slot_emit: %lld elements per part x max_count %d overflow a part's 32-bit total: use more parts", chunk,
                  max_count);
    const int vec = n % 4 == 0 && ((unsigned long long)pred & 15ull) == 0;
    hipLaunchKernelGGL(slot_emit_count_kernel, dim3(nparts, S), dim3(EMT), 0, (hipStream_t)s, table, emit, pred, (int)n,
                       (int)chunk, vec, (float)max_count, parts);
    BMC_CHECK_LAUNCH("bmc_slot_emit (count)");
    hipLaunchKernelGGL(slot_emit_write_kernel, dim3(nparts, S), dim3(EMT), 0, (hipStream_t)s, table, emit, pred, sH, sW, (int)n,
                       (int)chunk, vec, (float)max_count, (const unsigned*)parts);
    BMC_CHECK_LAUNCH("bmc_slot_emit (write)");
    return 0;
}
