// The LR event stream of an HR-only recording by integrate-and-fire over blocks of s x s HR pixels
// (bmc_hip.encodings.downsample_events, EventTrainSet.add_hr_recording, MultiStreamSR.open_hr_events); the contract is stated once
// in include/bmc_hip_downsample.h.
//
// The lesson of event_denoise.hip, where every band of the sensor walks the whole stream: here the events are grouped by the
// LR pixel they act on BEFORE anybody walks them.
//   keys    one lane per event writes the int32 id of its LR pixel (the sentinel h * w for an event that is not counted) and the
//           zero of fire;
//   group   one stable sort of the keys by the caller (torch.sort): the only stage that is not this file;
//   walk    one lane per LR pixel finds its segment of the sorted keys by two binary searches and runs the accumulator of the
//           contract over it in a register; a firing event's sign goes to fire[] at its ORIGINAL index, so the gather sees the
//           events in column order again without a second sort;
//   gather  the ordered compaction of slot_emit.hip in its two launches (chunk totals; every chunk adds the totals before it),
//           with wave_k.h's chunk range and sum of totals.  The tile scan is another one: an event fires once or not at
//           all, so a wave ranks its lanes with one ballot and a popcount instead of a prefix sum of counts, and the firing
//           events' indices are staged in LDS at their rank so that lane p stores output p.
// Integers decide everything; no global atomic, no workgroup waits for another, the grids are fixed by (n, h * w): the same bytes
// run after run.
#include "bmc_hip_downsample.h"
#include "wave_k.h"

namespace {

constexpr int LANES = BMC_DOWNSAMPLE_LANES;
constexpr int NW = LANES / 64;
constexpr int DTILE = BMC_DOWNSAMPLE_TILE;
constexpr int ROUNDS = DTILE / LANES;
static_assert(NW * 64 == LANES && ROUNDS * LANES == DTILE, "whole waves; a tile is whole rounds of one event per lane");

// grid ceil(n / LANES): lane l of workgroup g takes event g * LANES + l
__global__ __launch_bounds__(LANES) void event_downsample_keys_kernel(const short* __restrict__ xs, const short* __restrict__ ys,
                                                                      const double* __restrict__ ps, int n, int H, int W, int s,
                                                                      int w, int sentinel, int* __restrict__ keys,
                                                                      signed char* __restrict__ fire) {
    const long long i = (long long)blockIdx.x * LANES + threadIdx.x;
    if (i >= n) return;
    const int x = gld<short>(xs + i), y = gld<short>(ys + i);
    const double p = gld<double>(ps + i);
    const bool counted = x >= 0 && x < W && y >= 0 && y < H && (p > 0.0 || p < 0.0);
    gst<int>(keys + i, counted ? (y / s) * w + x / s : sentinel);
    gst<signed char>(fire + i, 0);
}

// the first j in [0, n) with sorted[j] >= q, n if there is none
__device__ __forceinline__ int lower_bound(const int* sorted, int n, int q) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (gld<int>(sorted + mid) < q) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// grid ceil(hw / LANES): one lane per LR pixel
__global__ __launch_bounds__(LANES) void event_downsample_walk_kernel(const int* __restrict__ sorted,
                                                                      const long long* __restrict__ perm,
                                                                      const double* __restrict__ ps, int n, int hw, int T,
                                                                      signed char* __restrict__ fire) {
    const long long q64 = (long long)blockIdx.x * LANES + threadIdx.x;
    if (q64 >= hw) return;
    const int q = (int)q64;
    const int lo = lower_bound(sorted, n, q), hi = lower_bound(sorted, n, q + 1);      // (q + 1 <= hw < 2^31 - 1)
    int a = 0;
    for (int j = lo; j < hi; ++j) {
        const long long i = gld<long long>(perm + j);
        if (i < 0 || i >= n) continue;                                  // not a permutation of 0 .. n-1: skipped, not followed
        a += gld<double>(ps + i) > 0.0 ? 1 : -1;
        if (a == T || a == -T) {
            gst<signed char>(fire + i, (signed char)(a > 0 ? 1 : -1));
            a = 0;
        }
    }
}

// grid (nparts): workgroup c counts the firing events of its chunk
__global__ __launch_bounds__(LANES) void event_downsample_total_kernel(const signed char* __restrict__ fire, int n, int chunk,
                                                                       unsigned* __restrict__ parts) {
    __shared__ unsigned wsum[NW];
    const int part = blockIdx.x, tid = threadIdx.x;
    const PartRange r = part_range(part, chunk, n);
    unsigned acc = 0u;
    for (int i = r.lo + tid; i < r.hi; i += LANES) acc += gld<signed char>(fire + i) != 0 ? 1u : 0u;
    acc = block_fold<NW>(acc, Sum(), wsum);
    if (tid == 0) gst<unsigned>(parts + part, acc);
}

// grid (nparts): workgroup c places its chunk's firing events behind those of the chunks before it
__global__ __launch_bounds__(LANES) void event_downsample_write_kernel(const short* __restrict__ xs, const short* __restrict__ ys,
                                                                       const double* __restrict__ ts,
                                                                       const signed char* __restrict__ fire, int n, int chunk, int s,
                                                                       const unsigned* __restrict__ parts, short* __restrict__ out_xs,
                                                                       short* __restrict__ out_ys, double* __restrict__ out_ts,
                                                                       double* __restrict__ out_ps, long long cap,
                                                                       long long* __restrict__ count) {
    __shared__ int src[DTILE];                    // rank inside the tile -> (tile-local event index << 1) | (fires -1)
    __shared__ unsigned wcnt[ROUNDS * NW];        // firing events of (round, wave), in the tile's event order
    __shared__ unsigned long long red[NW];
    const int part = blockIdx.x, nparts = gridDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // events of the chunks before this one; workgroup 0 has none before it and adds ALL chunks instead: the count
    const unsigned long long before = sum_parts<NW>(parts, part == 0 ? nparts : part, red);
    long long gpos = (long long)before;
    if (part == 0) {
        if (tid == 0) gst<long long>(count, gpos);
        gpos = 0;
    }
    const PartRange r = part_range(part, chunk, n);
    for (int tb = r.lo; tb < r.hi; tb += DTILE) {                     // (uniform over the workgroup)
        signed char f[ROUNDS];
        unsigned below[ROUNDS];
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) {                            // round k: event tb + k * LANES + tid
            const int i = tb + k * LANES + tid;
            f[k] = i < r.hi ? gld<signed char>(fire + i) : (signed char)0;
            const unsigned long long m = __ballot(f[k] != 0);
            below[k] = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[k * NW + wave] = (unsigned)__popcll(m);
        }
        __syncthreads();
        unsigned ttot = 0u;                                           // the tile's event order is (round, wave, lane)
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) {
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                if (w == wave && f[k] != 0) src[ttot + below[k]] = ((k * LANES + tid) << 1) | (f[k] < 0 ? 1 : 0);
                ttot += wcnt[k * NW + w];
            }
        }
        __syncthreads();
        for (unsigned p = tid; p < ttot; p += LANES) {                // output position p of the tile <- its event
            const long long pos = gpos + p;
            if (pos >= cap) break;                                    // (positions only grow with p)
            const int v = src[p];
            const int i = tb + (v >> 1);
            gst<short>(out_xs + pos, (short)(gld<short>(xs + i) / s));
            gst<short>(out_ys + pos, (short)(gld<short>(ys + i) / s));
            gst<unsigned long long>(out_ts + pos, gld<unsigned long long>(ts + i));
            gst<double>(out_ps + pos, (v & 1) ? -1.0 : 1.0);
        }
        gpos += ttot;
        __syncthreads();                                              // src and wcnt are free for the next tile
    }
}

static inline long long chunk_of(long long n) {
    const long long m = n > 0 ? n : 1;
    const long long per = (m + BMC_DOWNSAMPLE_MAX_PARTS - 1) / BMC_DOWNSAMPLE_MAX_PARTS;
    return (per + DTILE - 1) / DTILE * DTILE;
}

static inline int nparts_of(long long n) {
    const long long c = chunk_of(n), p = (n + c - 1) / c;
    return (int)(p < 1 ? 1 : p);
}

// the checks the three entry points share; -> 0 and *hw = h * w, or -1 with the error set
static inline int downsample_geometry(const char* who, long long n, int H, int W, int s, int* w, int* hw) {
    BMC_CHECK_ARG(n >= 0 && n < (1ll << 31), "%s: %lld events are not supported (0 <= n < 2^31)", who, n);
    BMC_CHECK_ARG(H >= 1 && W >= 1, "%s: a sensor of %d x %d pixels", who, H, W);
    BMC_CHECK_ARG(s >= 1 && s <= BMC_DOWNSAMPLE_MAX_SCALE, "%s: scale %d is outside 1 .. %d", who, s, BMC_DOWNSAMPLE_MAX_SCALE);
    const long long h = (H + (long long)s - 1) / s, ww = (W + (long long)s - 1) / s;
    BMC_CHECK_ARG(h * ww < (1ll << 31) - 1, "%s: %lld x %lld LR pixels are not below 2^31 - 1", who, h, ww);
    *w = (int)ww;
    *hw = (int)(h * ww);
    return 0;
}

}  // namespace

extern "C" long long bmc_event_downsample_capacity(long long n, int T) {
    if (n < 0 || n >= (1ll << 31) || T < 1 || T > BMC_DOWNSAMPLE_MAX_THRESHOLD) return -1;
    return n / T;
}

extern "C" long long bmc_event_downsample_chunk(long long n) {
    if (n < 0 || n >= (1ll << 31)) return -1;
    return chunk_of(n);
}

extern "C" long long bmc_event_downsample_scratch_bytes(long long n) {
    if (n < 0 || n >= (1ll << 31)) return -1;
    return (4ll * nparts_of(n) + 7) / 8 * 8;
}

extern "C" int bmc_event_downsample_keys(const short* xs, const short* ys, const double* ps, long long n, int H, int W, int s,
                                         int* keys, signed char* fire, bmc_stream_t stream) {
    int w, hw;
    if (downsample_geometry("bmc_event_downsample_keys", n, H, W, s, &w, &hw)) return -1;
    BMC_CHECK_ARG(n == 0 || (xs && ys && ps && keys && fire), "bmc_event_downsample_keys: null columns");
    if (n == 0) return 0;
    hipLaunchKernelGGL(event_downsample_keys_kernel, dim3((unsigned)((n + LANES - 1) / LANES)), dim3(LANES), 0, (hipStream_t)stream,
                       xs, ys, ps, (int)n, H, W, s, w, hw, keys, fire);
    BMC_CHECK_LAUNCH("bmc_event_downsample_keys");
    return 0;
}

extern "C" int bmc_event_downsample_walk(const int* sorted, const long long* perm, const double* ps, long long n, int H, int W,
                                         int s, int T, signed char* fire, bmc_stream_t stream) {
    int w, hw;
    if (downsample_geometry("bmc_event_downsample_walk", n, H, W, s, &w, &hw)) return -1;
    BMC_CHECK_ARG(T >= 1 && T <= BMC_DOWNSAMPLE_MAX_THRESHOLD, "bmc_event_downsample_walk: threshold %d is outside 1 .. %d", T,
                  BMC_DOWNSAMPLE_MAX_THRESHOLD);
    BMC_CHECK_ARG(n == 0 || (sorted && perm && ps && fire), "bmc_event_downsample_walk: null columns");
    if (n == 0) return 0;
    hipLaunchKernelGGL(event_downsample_walk_kernel, dim3((unsigned)(((long long)hw + LANES - 1) / LANES)), dim3(LANES), 0,
                       (hipStream_t)stream, sorted, perm, ps, (int)n, hw, T, fire);
    BMC_CHECK_LAUNCH("bmc_event_downsample_walk");
    return 0;
}

extern "C" int bmc_event_downsample_gather(const short* xs, const short* ys, const double* ts, const signed char* fire, long long n,
                                           int s, short* out_xs, short* out_ys, double* out_ts, double* out_ps, long long capacity,
                                           long long* count, unsigned* scratch, bmc_stream_t stream) {
    const char* const who = "bmc_event_downsample_gather";
    BMC_CHECK_ARG(n >= 0 && n < (1ll << 31), "%s: %lld events are not supported (0 <= n < 2^31)", who, n);
    BMC_CHECK_ARG(s >= 1 && s <= BMC_DOWNSAMPLE_MAX_SCALE, "%s: scale %d is outside 1 .. %d", who, s, BMC_DOWNSAMPLE_MAX_SCALE);
    BMC_CHECK_ARG(capacity >= 0, "%s: a capacity of %lld", who, capacity);
    BMC_CHECK_ARG(count && scratch, "%s: null count or scratch", who);
    BMC_CHECK_ARG(n == 0 || (xs && ys && ts && fire), "%s: null columns", who);
    BMC_CHECK_ARG(capacity == 0 || (out_xs && out_ys && out_ts && out_ps), "%s: null output columns", who);
    BMC_CHECK_ARG(((unsigned long long)scratch & 7ull) == 0, "%s: scratch is not 8-byte aligned", who);
    const int chunk = (int)chunk_of(n), nparts = nparts_of(n);
    hipLaunchKernelGGL(event_downsample_total_kernel, dim3(nparts), dim3(LANES), 0, (hipStream_t)stream, fire, (int)n, chunk, scratch);
    BMC_CHECK_LAUNCH("bmc_event_downsample_gather (totals)");
    hipLaunchKernelGGL(event_downsample_write_kernel, dim3(nparts), dim3(LANES), 0, (hipStream_t)stream, xs, ys, ts, fire, (int)n,
                       chunk, s, (const unsigned*)scratch, out_xs, out_ys, out_ts, out_ps, capacity, count);
    BMC_CHECK_LAUNCH("bmc_event_downsample_gather (write)");
    return 0;
}
