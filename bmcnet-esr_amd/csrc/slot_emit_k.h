// What the event-output files share (internal): slot_emit.hip (bmc_slot_emit), slot_emit_timed.hip (bmc_slot_emit_timed /
// _clocked) and slot_emit_trimmed.hip (bmc_slot_emit_trimmed).  A timed stream is "the events of slot_emit.hip, with times", so the quantisation rule, the walk over a slot's
// prediction and the decoding of an element into an event exist once, here.  slot_emit.hip describes the algorithm.
#pragma once
#include "wave_k.h"

namespace {

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
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = quant(v[k], mc);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < hi) q[k] = quant(gld<float>(ps + i + k), mc);
    }
}

// the events of a lane's 4 elements
__device__ __forceinline__ unsigned sum_q4(const unsigned (&q)[4]) {
    unsigned t = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) t += q[k];
    return t;
}

// the slot emits this window: it is active and its emit entry has columns (uniform over the workgroup).  E: bmc_slot_emit_t
// or bmc_slot_emit_timed_t (the same leading fields)
template <class E>
__device__ __forceinline__ bool emits(const bmc_slot_t* table, const E* emit, int s) {
    return (gld<int>(&table[s].flags) & BMC_SLOT_ACTIVE) && gld<const float*>(&table[s].frames) != nullptr &&
           gld<short*>(&emit[s].xs) != nullptr;
}

// every event of an element is emitted: the `pick` of tile_scan that changes nothing
struct AllEvents {
    __device__ __forceinline__ void operator()(unsigned (&)[4], int) const {}
};

// One tile of a part: this lane brings the q of elements tb + 4 * tid .. + 3 (block_scan_excl over the lanes' sums);
// excl[TILE] <- the exclusive prefix of q inside the tile, -> the tile's events.  wtot: NW words of LDS.  Called by all 256
// threads; excl is complete when it returns.  pick(q, e): may lower the q of the tile's elements e .. e+3 before they are
// scanned (the trimmed output emits the first keep[q] events of an element).
template <class Pick = AllEvents>
__device__ __forceinline__ unsigned tile_scan(const float* ps, int tb, int hi, bool vec, float mc, unsigned* excl, unsigned* wtot,
                                              int tid, Pick pick = Pick()) {
    unsigned q[4], ttot;
    load_q4(ps, tb + 4 * tid, hi, vec, mc, q);
    pick(q, 4 * tid);
    unsigned e = block_scan_excl<NW>(sum_q4(q), wtot, &ttot);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        excl[4 * tid + k] = e;
        e += q[k];
    }
    __syncthreads();
    return ttot;
}

// the element of the tile that owns output position p < ttot: the largest e with excl[e] <= p (its q is > 0)
__device__ __forceinline__ int tile_owner(const unsigned* excl, unsigned p) {
    int e = 0;
#pragma unroll
    for (int step = TILE / 2; step > 0; step >>= 1)
        if (excl[e + step] <= p) e += step;
    return e;
}

// flat element idx of [2][sH][sW] (hw = sH * sW) -> its event (x, sH-1-row, +1 / -1 by channel) at position pos of the columns
__device__ __forceinline__ void store_event(short* xs, short* ys, signed char* pol, long long pos, unsigned idx, int sH, int sW,
                                            unsigned hw) {
    const unsigned c = idx >= hw ? 1u : 0u, rem = idx - c * hw, row = rem / (unsigned)sW, x = rem - row * (unsigned)sW;
    gst<short>(xs + pos, (short)x);
    gst<short>(ys + pos, (short)(sH - 1 - (int)row));
    gst<signed char>(pol + pos, (signed char)(c ? -1 : 1));
}

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int T2 = BMC_SLOT_EMIT_TIMED_BLOCK;   // records per workgroup of the high-digit pass

// One step of the stable split: every lane brings at most one record (digit d; !valid: none), the records of a step are in
// sequence order by (wave, lane) and the steps of a workgroup follow one another.  run[d] = the position of the next record
// of digit d (it starts at the workgroup's offset for the digit); stepc[w][d] = 0 between steps.  Called by all 256 threads.
__device__ __forceinline__ unsigned place(unsigned* run, unsigned (*stepc)[256], bool valid, unsigned d, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned long long peers = __ballot(valid);                       // -> the lanes of this wave with the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long m = __ballot(valid && bit);
        peers &= bit ? m : ~m;
    }
    const unsigned below = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
    if (valid && below == 0u) stepc[wave][d] = (unsigned)__popcll(peers);
    __syncthreads();
    unsigned r = 0u;
    if (valid) {
        r = run[d] + below;
#pragma unroll
        for (int w = 0; w < NW - 1; ++w)
            if (w < wave) r += stepc[w][d];
    }
    __syncthreads();
    run[tid] += stepc[0][tid] + stepc[1][tid] + stepc[2][tid] + stepc[3][tid];     // thread t owns digit t
    stepc[0][tid] = stepc[1][tid] = stepc[2][tid] = stepc[3][tid] = 0u;
    __syncthreads();
    return r;
}

// float64 time of event j of n on the clock [t_first, t_first + dt]: tau from the REDUCED fraction (Euclid on 8-bit values: at
// most 12 steps for j <= n - 1 <= 254), then a multiply and an add that are rounded separately (no fma contraction).
__device__ __forceinline__ double clock_time(double t_first, double dt, unsigned j, unsigned nq) {
#pragma clang fp contract(off)
    double tau = BMC_EVENT_T0;
    if (nq > 1u) {
        unsigned a = j, b = nq - 1u;
        for (int it = 0; it < 16 && b != 0u; ++it) {
            const unsigned r = a % b;
            a = b;
            b = r;
        }
        tau = BMC_EVENT_T0 + (BMC_EVENT_T1 - BMC_EVENT_T0) * (double)(j / a) / (double)((nq - 1u) / a);
    }
    const double span = tau * dt;
    return t_first + span;
}

// elements per slot and per part of a launch, and whether a lane may load its 4 elements as one f32x4
struct EmitGeom {
    int n, chunk, vec;
};
// The argument checks that bmc_slot_emit and bmc_slot_emit_timed / _clocked share (`who` names the entry point; max_count has
// been checked by the caller, whose bound it is) -> 0 and the geometry, or -1 with the error set.
static inline int emit_geometry(const char* who, const void* table, const void* emit, const float* pred, const unsigned* parts,
                                int S, int sH, int sW, int max_count, int nparts, EmitGeom* g) {
    BMC_CHECK_ARG(table && emit && pred && parts && S >= 1 && S <= BMC_MAX_SLOTS, "%s: bad arguments", who);
    BMC_CHECK_ARG(sH >= 1 && sW >= 1 && sH <= 32767 && sW <= 32767,
                  "%s: sH, sW must be 1 .. 32767 (coordinates are int16; got %d x %d)", who, sH, sW);
    BMC_CHECK_ARG(nparts >= 1 && nparts <= BMC_SLOT_EMIT_MAX_PARTS, "%s: 1 <= nparts <= %d (got %d)", who,
                  BMC_SLOT_EMIT_MAX_PARTS, nparts);
    BMC_CHECK_ARG(((unsigned long long)pred & 3ull) == 0, "%s: pred must be 4-byte aligned", who);
    const long long n = 2ll * sH * sW;                                // < 2^31 for sH, sW <= 32767
    const long long chunk = ((n + nparts - 1) / nparts + 3) / 4 * 4;
    BMC_CHECK_ARG(chunk * max_count < (1ll << 32),
                  "%s: %lld elements per part x max_count %d overflow a part's 32-bit total: use more parts", who, chunk,
                  max_count);
    g->n = (int)n;
    g->chunk = (int)chunk;
    g->vec = n % 4 == 0 && ((unsigned long long)pred & 15ull) == 0;
    return 0;
}

}  // namespace

// What slot_emit_trimmed.hip (bmc_slot_emit_trimmed) shares with slot_emit_timed.hip, which defines the three functions: the
// argument checks and the scratch layout of a timed call, and the launches that are the same kernels in both -- the first scan
// and the high-digit pass.  Host code, internal to the library.
struct EmitTimedPlan {
    const bmc_slot_t* table;
    const bmc_slot_emit_timed_t* emit;
    const bmc_slot_clock_t* clock;
    int S, sH, sW, nparts, blocks, hrows;
    EmitGeom g;
    float mc;                           // max_count
    const float* pred;
    unsigned* parts;
    const unsigned short* rank;
    u32x2* rec;                         // the scratch: records [S][wcap], totals [S], digit bases [S][256], histograms [S][hrows][256]
    unsigned long long* tot;
    unsigned* dbase;
    unsigned* hist;
    long long wcap;
    hipStream_t st;
};
// -> 0 and the plan, or -1 with the error set (`who` names the entry point)
__attribute__((visibility("hidden"))) int bmc_emit_timed_plan(const char* who, const bmc_slot_t* table, const bmc_slot_emit_timed_t* emit,
                                                              const bmc_slot_clock_t* clock, int S, const float* pred, int sH, int sW,
                                                              int max_count, int nparts, unsigned* parts,
                                                              const unsigned short* rank_table, void* scratch,
                                                              long long window_capacity, bmc_stream_t s, EmitTimedPlan* p);
// scan 1 (after the count launch): the slot's total, *index_out, offsets over (digit, part) -> 0, or -2
__attribute__((visibility("hidden"))) int bmc_emit_timed_scan_parts(const EmitTimedPlan& p);
// histogram, scan 2, scatter (after the expand launch) -> 0, or -2
__attribute__((visibility("hidden"))) int bmc_emit_timed_high_pass(const EmitTimedPlan& p);
