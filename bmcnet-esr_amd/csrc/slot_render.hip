// Event-count images of multi-stream inference (bmcnet-esr_amd/infer.py::MultiStreamSR(render=...)); the contract is stated once
// in include/bmc_hip.h ("event-count images").  bmc_slot_render turns a [2][h][w] count image of every slot with a render entry
// into the uint8 [h][w][3] image the reference's plot_event_cnt returns (myutils/vis_events/matplotlib_plot_events.py:125-248),
// in TWO launches for all slots:
//   select  grid (2, S), one workgroup of 1 024 lanes per (channel, slot): NumPy's 1st and 99th percentile of the plane need
//           four order statistics (the ranks come from the host: they depend on h * w alone).  An 8-bit radix select over
//           order-preserving unsigned keys of the float32 values finds all four at once, top digit first, four passes over the
//           plane: one 256-bin LDS histogram per tracked rank (ranks whose prefixes still agree share the first one's), a wave per
//           rank scans its histogram and picks the digit.  Lane 0 restates NumPy's float32 lerp and writes (min, max) to scratch.
//           Count images are mostly one value, so a wave first folds the lanes that agree with its first lane into ONE integer
//           LDS atomic; the rest add one by one.
//   colour  grid (nparts, S): normalise, clip, colour, pack: a lane owns four pixels = three 32-bit words of the output.
// Integer LDS atomics only, no global atomics, no workgroup waits for another, grids fixed by the arguments: the same bytes run
// after run, capturable.  The float32 arithmetic that decides a byte is written with __f*_rn intrinsics: never contracted into an
// FMA, the division correctly rounded.  Pointers read from the tables go through address-space(1) casts (slot_k.h).
#include "wave_k.h"

namespace {

constexpr int RT = 1024;            // select: threads per workgroup
constexpr int NR = 4;               // tracked ranks: floor and floor + 1 of the two virtual indices
constexpr int CT = 256;             // colour: threads per workgroup

struct RenderRanks {
    unsigned k[NR];                 // k_lo, k_lo + 1, k_hi, k_hi + 1 (0-based, < n)
    float g[2];                     // NumPy's gamma of the two percentiles
};

__device__ __forceinline__ bool slot_active(const bmc_slot_t* table, int s) {
    return (gld<int>(&table[s].flags) & BMC_SLOT_ACTIVE) && gld<const float*>(&table[s].frames) != nullptr;
}

// order-preserving unsigned image of a float32 (-0.0 orders as +0.0) and its inverse
__device__ __forceinline__ unsigned float_key(float v) {
    const unsigned b = v == 0.f ? 0u : __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// numpy.lib._function_base_impl._lerp in float32
__device__ __forceinline__ float lerp_np(float a, float b, float t) {
    const float d = __fsub_rn(b, a);
    return t >= 0.5f ? __fsub_rn(b, __fmul_rn(d, __fsub_rn(1.f, t))) : __fadd_rn(a, __fmul_rn(d, t));
}

template <class T>
__device__ __forceinline__ T pick(T a0, T a1, T a2, T a3, int r) {  // element r of four values, without a runtime register index
    return r == 0 ? a0 : (r == 1 ? a1 : (r == 2 ? a2 : a3));
}

// h[bin] += 1 for every lane with m, called by whole waves: the lanes that share the first such lane's bin add once, together
__device__ __forceinline__ void wave_hist_add(unsigned* h, unsigned bin, bool m, int lane) {
    const unsigned long long todo = __ballot(m);
    if (todo == 0ull) return;
    const int first = __ffsll((long long)todo) - 1;
    const unsigned b = (unsigned)__shfl((int)bin, first);
    const unsigned long long same = __ballot(m && bin == b);
    if (lane == first)
        atomicAdd(&h[b], (unsigned)__popcll(same));
    else if (m && bin != b)
        atomicAdd(&h[bin], 1u);
}

// grid (2, S): blockIdx.x is the channel, blockIdx.y the slot
__global__ __launch_bounds__(RT) void slot_render_select_kernel(const bmc_slot_t* __restrict__ table,
                                                                const bmc_slot_render_t* __restrict__ render, int n, int round,
                                                                RenderRanks rr, float* __restrict__ minmax) {
    __shared__ unsigned hist[NR][256];
    __shared__ unsigned sel[NR][2];
    const int c = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!slot_active(table, s)) return;                              // (uniform over the workgroup)
    const float* const src = gld<const float*>(&render[s].src);
    if (src == nullptr) return;
    const float* const plane = src + (long long)c * n;
    unsigned prefix[NR] = {0u, 0u, 0u, 0u}, k[NR] = {rr.k[0], rr.k[1], rr.k[2], rr.k[3]}, pmask = 0u;
#pragma unroll
    for (int shift = 24; shift >= 0; shift -= 8) {
        // rank r counts into the histogram of rep[r], the first of its run of equal prefixes (neighbouring ranks mostly agree)
        int rep[NR];
        rep[0] = 0;
#pragma unroll
        for (int r = 1; r < NR; ++r) rep[r] = prefix[r] == prefix[r - 1] ? rep[r - 1] : r;
        for (int i = tid; i < NR * 256; i += RT) (&hist[0][0])[i] = 0u;
        __syncthreads();
        for (int base = 0; base < n; base += RT) {                   // (every lane makes every trip: the ballots need whole waves)
            const int p = base + tid;
            const bool in = p < n;
            unsigned key = 0u;
            if (in) {
                float v = gld<float>(plane + p);
                if (round) v = rintf(v);
                key = float_key(v);
            }
            const unsigned top = key & pmask, bin = (key >> shift) & 255u;
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (rep[r] == r) wave_hist_add(hist[r], bin, in && top == prefix[r], lane);
        }
        __syncthreads();
        if (wave < NR) {                                             // wave r: the digit of rank r; a lane holds four bins
            const unsigned* const h = hist[pick(rep[0], rep[1], rep[2], rep[3], wave)];
            const DigitPick dp = digit_pick(h, pick(k[0], k[1], k[2], k[3], wave), lane);
            if (dp.found) {                                          // exactly one lane
                sel[wave][0] = dp.bin;
                sel[wave][1] = dp.rank;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            prefix[r] |= sel[r][0] << shift;
            k[r] = sel[r][1];
        }
        pmask |= 255u << shift;
    }
    if (tid == 0) {
        float* const mm = minmax + ((long long)s * 2 + c) * 2;
        mm[0] = lerp_np(key_float(prefix[0]), key_float(prefix[1]), rr.g[0]);
        mm[1] = lerp_np(key_float(prefix[2]), key_float(prefix[3]), rr.g[1]);
    }
}

__device__ __forceinline__ float norm_clip(float v, bool norm, float mn, float range) {
    if (norm) v = __fdiv_rn(__fsub_rn(v, mn), range);
    return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
}
__device__ __forceinline__ unsigned to_byte(float c) { return (unsigned)(int)((double)c * 255.0); }

// grid (nparts, S), CT threads; a lane owns groups of four pixels (twelve bytes of the image)
__global__ __launch_bounds__(CT) void slot_render_colour_kernel(const bmc_slot_t* __restrict__ table,
                                                                const bmc_slot_render_t* __restrict__ render, int n, int round,
                                                                const float* __restrict__ minmax) {
    const int s = blockIdx.y;
    if (!slot_active(table, s)) return;
    const float* const src = gld<const float*>(&render[s].src);
    unsigned char* const dst = gld<unsigned char*>(&render[s].dst);
    if (src == nullptr || dst == nullptr) return;
    const float* const mm = minmax + 4ll * s;
    const float min0 = mm[0], max0 = mm[1], min1 = mm[2], max1 = mm[3];
    const float mx = max0 > max1 ? max0 : max1;
    const bool norm0 = min0 != mx, norm1 = min1 != mx;               // (otherwise the channel stays as it is: the reference's quirk)
    const float range0 = __fsub_rn(mx, min0), range1 = __fsub_rn(mx, min1);
    const bool words = ((unsigned long long)dst & 3ull) == 0ull;
    const int groups = (n + 3) / 4;
    for (int g = blockIdx.x * CT + threadIdx.x; g < groups; g += gridDim.x * CT) {
        const int p0 = 4 * g, cnt = n - p0 < 4 ? n - p0 : 4;
        unsigned px[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            px[j][0] = px[j][1] = px[j][2] = 0u;
            if (j < cnt) {
                float a = gld<float>(src + p0 + j), b = gld<float>(src + (long long)n + p0 + j);
                if (round) { a = rintf(a); b = rintf(b); }
                const float p = norm_clip(a, norm0, min0, range0), q = norm_clip(b, norm1, min1, range1);
                float c0 = 1.f, c1 = 1.f, c2 = 1.f;                  // the reference's BGR triple
                if (p > 0.f && (q == 0.f || p >= q)) {
                    c1 = c2 = __fsub_rn(1.f, p);
                } else if (q > 0.f) {
                    c0 = c1 = __fsub_rn(1.f, q);
                }
                px[j][0] = to_byte(c2);                              // COLOR_BGR2RGB: the triple reversed
                px[j][1] = to_byte(c1);
                px[j][2] = to_byte(c0);
            }
        }
        unsigned char* const o = dst + 3ll * p0;
        if (words && cnt == 4) {
            gst<unsigned>(o, px[0][0] | px[0][1] << 8 | px[0][2] << 16 | px[1][0] << 24);
            gst<unsigned>(o + 4, px[1][1] | px[1][2] << 8 | px[2][0] << 16 | px[2][1] << 24);
            gst<unsigned>(o + 8, px[2][2] | px[3][0] << 8 | px[3][1] << 16 | px[3][2] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) {
                    gst<unsigned char>(o + 3 * j, (unsigned char)px[j][0]);
                    gst<unsigned char>(o + 3 * j + 1, (unsigned char)px[j][1]);
                    gst<unsigned char>(o + 3 * j + 2, (unsigned char)px[j][2]);
                }
        }
    }
}

// NumPy's placement of percentile q of n float32 values (method "linear"): q / 100 and the virtual index (n - 1) * q are FLOAT32
// (np.percentile divides by the array's own float32(100)); n - 1 < 2^24 is exact.  -> rank of the lower neighbour, its gamma
void percentile_rank(int n, float q, unsigned& lo, unsigned& hi, float& gamma) {
    const float last = (float)(n - 1);
    const volatile float vi = last * q;                              // (volatile: one float32 product, rounded once)
    const float v = vi;
    if (v >= last) {
        lo = hi = (unsigned)(n - 1);
        gamma = 0.f;
    } else {
        const float f = __builtin_floorf(v);
        lo = (unsigned)f;
        hi = lo + 1u;
        gamma = v - f;
    }
}

}  // namespace

extern "C" int bmc_slot_render(const bmc_slot_t* table, const bmc_slot_render_t* render, int S, int h, int w, int round,
                               int nparts, float* scratch, bmc_stream_t s) {
    BMC_CHECK_ARG(table && render && scratch && S >= 1 && S <= BMC_MAX_SLOTS && h > 0 && w > 0 && nparts >= 1 &&
                      nparts <= BMC_SLOT_RENDER_MAX_PARTS,
                  "bmc_slot_render: bad arguments");
    BMC_CHECK_ARG((long long)h * w <= BMC_SLOT_RENDER_MAX_PIXELS, "bmc_slot_render: images of %d x %d pixels are not supported", h,
                  w);
    const int n = h * w;
    RenderRanks rr;
    percentile_rank(n, 0.01f, rr.k[0], rr.k[1], rr.g[0]);
    percentile_rank(n, 0.99f, rr.k[2], rr.k[3], rr.g[1]);
    hipLaunchKernelGGL(slot_render_select_kernel, dim3(2, S), dim3(RT), 0, (hipStream_t)s, table, render, n, round ? 1 : 0, rr,
                       scratch);
    BMC_CHECK_LAUNCH("bmc_slot_render (select)");
    hipLaunchKernelGGL(slot_render_colour_kernel, dim3(nparts, S), dim3(CT), 0, (hipStream_t)s, table, render, n, round ? 1 : 0,
                       (const float*)scratch);
    BMC_CHECK_LAUNCH("bmc_slot_render (colour)");
    return 0;
}
