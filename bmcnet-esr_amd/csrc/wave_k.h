// Cross-lane primitives of the event and slot kernels (internal): the folds, scans and the radix digit pick that those kernels
// share, each written once.  Workgroups are one-dimensional and made of whole waves of 64 lanes; NWAVES is their number.  No
// primitive owns LDS: the caller passes the words, and where it reuses them it places the barrier that ends their previous
// reading.  Fold order, part of the float64 users' bit-for-bit contracts: the lanes of a wave in the fixed tree of offsets
// 32, 16, .. 1, then the waves left to right, ((w0 op w1) op w2) op w3.
#pragma once
#include "slot_k.h"

namespace {

struct Sum { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct Max { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; } };
struct Min { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; } };

// Called by whole waves; no barrier.  -> the wave's 64 values folded in the fixed tree, on lane 0 (other lanes: partial folds).
template <class T, class Op>
__device__ __forceinline__ T wave_fold(T v, Op op) {
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_down(v, o));
    return v;
}

// The two halves of a workgroup fold, for callers that fold several values across ONE barrier of their own.
// Called by whole waves, lds[wave] free to write; no barrier.  lds[wave] <- the wave's fold.
template <class T, class Op>
__device__ __forceinline__ void wave_fold_to(T v, Op op, T* lds) {
    v = wave_fold(v, op);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
}
// Any thread, after the barrier that completes lds[0 .. N).  -> the N words folded left to right.
template <int N, class T, class Op>
__device__ __forceinline__ T lds_fold(const T* lds, Op op) {
    T r = lds[0];
#pragma unroll
    for (int w = 1; w < N; ++w) r = op(r, lds[w]);
    return r;
}

// Called by all threads, lds[0 .. NWAVES) free to write; holds one barrier.  -> the workgroup's values folded, on thread 0
// (other threads: unspecified).
template <int NWAVES, class T, class Op>
__device__ __forceinline__ T block_fold(T v, Op op, T* lds) {
    wave_fold_to(v, op, lds);
    __syncthreads();
    return threadIdx.x == 0 ? lds_fold<NWAVES>(lds, op) : v;
}
// As block_fold, with the result on EVERY thread.
template <int NWAVES, class T, class Op>
__device__ __forceinline__ T block_fold_all(T v, Op op, T* lds) {
    wave_fold_to(v, op, lds);
    __syncthreads();
    return lds_fold<NWAVES>(lds, op);
}

// Called by whole waves; no barrier.  -> v of this lane and of the lanes below it in the wave.
template <class T>
__device__ __forceinline__ T wave_scan_incl(T v) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// Called by all threads, lds[0 .. NWAVES) free to write; holds one barrier.  -> the sum of v over the threads below this one
// (thread order = wave, lane); *total = the sum over the workgroup, on every thread.
template <int NWAVES, class T>
__device__ __forceinline__ T block_scan_excl(T v, T* lds, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T inc = wave_scan_incl(v);
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    T off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
        const T t = lds[w];
        if (w < wave) off += t;
        tot += t;
    }
    *total = tot;
    return off + inc - v;
}

// One digit of an 8-bit radix select.  Called by ONE whole wave after the barrier that completes hist[0 .. 256); no barrier.
// k < the histogram's total is a 0-based rank counted from bin 0; a lane holds four bins.  On exactly one lane `found` is set:
// there bin holds rank k and rank = k - (the keys in the bins below it).
struct DigitPick {
    unsigned bin, rank;
    bool found;
};
__device__ __forceinline__ DigitPick digit_pick(const unsigned* hist, unsigned k, int lane) {
    const unsigned b0 = hist[4 * lane], b1 = hist[4 * lane + 1], b2 = hist[4 * lane + 2], b3 = hist[4 * lane + 3];
    const unsigned sum = b0 + b1 + b2 + b3, inc = wave_scan_incl(sum);
    unsigned d = 0u, cum = inc - sum;
    const bool found = cum <= k && k < inc;
    if (k >= cum + b0) { cum += b0; d = 1u; }
    if (d == 1u && k >= cum + b1) { cum += b1; d = 2u; }
    if (d == 2u && k >= cum + b2) { cum += b2; d = 3u; }
    return DigitPick{4u * lane + d, k - cum, found};
}

// part p of a grid of parts owns elements [lo, hi) = [p * chunk, min(n, (p+1) * chunk)) of n
struct PartRange {
    int lo, hi;
};
__device__ __forceinline__ PartRange part_range(int part, int chunk, int n) {
    const long long lo64 = (long long)part * chunk;
    return PartRange{(int)(lo64 < n ? lo64 : n), (int)(lo64 + chunk < n ? lo64 + chunk : n)};
}

// pp[0] + .. + pp[cnt - 1] (part totals) in every thread.  red: NWAVES words of LDS, free to write.  Called by all threads.
template <int NWAVES>
__device__ __forceinline__ unsigned long long sum_parts(const unsigned* pp, int cnt, unsigned long long* red) {
    constexpr int THREADS = 64 * NWAVES;
    unsigned long long acc = 0ull;
    for (int j = threadIdx.x; j < cnt; j += THREADS) acc += gld<unsigned>(pp + j);
    return block_fold_all<NWAVES>(acc, Sum(), red);
}

}  // namespace
