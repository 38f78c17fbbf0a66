// Recording slots of multi-stream inference (bmcnet-esr_amd/infer.py::MultiStreamSR): S independent recordings share one
// batched forward pass, each in a slot of the batch.  Per window, whatever S is:
//   bmc_slot_stage    gathers each slot's input window into the static batch input and loads the recurrent state from the
//                     pool (exact zeros for a slot that starts a recording or is empty; a bf16 pool is widened to fp32);
//   bmc_slot_commit   writes the model's new state back into the pool (a bf16 pool: rounded to nearest-even, bit-identical
//                     to tensor.to(torch.bfloat16)) and, where asked, the slot's prediction to the caller's buffer;
//   bmc_slot_metrics  the two metrics of infer_BMCNet.py:76-85 as sums of squares: `nparts` workgroups per slot, each the
//                     fixed-order sum of a fixed set of elements, written as partial sums that the host adds in a fixed
//                     order when it reads them (no atomics: bit-reproducible, and a slot's sums do not depend on its
//                     neighbours).
// Self-ensemble (include/bmc_hip.h states the contract) is table data behind the first two: stage gathers the frames of a slot
// with an orientation code oriented, commit merges the predictions of a group of K slots into its leader's row of the model's
// output, in place, which the metrics and the later slot kernels then read.
// The per-slot table (bmc_slot_t) lives in device memory, so a captured graph replays with whatever the host copied into it.
// Pointers read from the table are generic to the compiler: every access goes through an address-space(1) cast (global_*
// instructions, never flat_*).
#include "slot_k.h"
#include "cubic_taps.h"

namespace {

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf2f(unsigned short b) { return __uint_as_float((unsigned)b << 16); }
// c10::BFloat16's round_to_nearest_even: NaN -> 0x7fc0, otherwise add 0x7fff + lsb and truncate
__device__ __forceinline__ unsigned short f2bf(float f) {
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)0x7fc0;
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// a table entry, field by field (a struct copy out of address space 1 has no constructor)
__device__ __forceinline__ bmc_slot_t load_slot(const bmc_slot_t* table, int s) {
    const bmc_slot_t* const p = table + s;
    bmc_slot_t e;
    e.frames = gld<const float*>(&p->frames);
    e.gt = gld<const float*>(&p->gt);
    e.keep = gld<float*>(&p->keep);
    e.result = gld<double*>(&p->result);
    e.flags = gld<int>(&p->flags);
    e.pad_ = 0;
    return e;
}

// bits 2..4 of the flags: the slot's orientation code (bit 0 horizontal, 1 vertical, 2 polarity)
__device__ __forceinline__ int orient_of(int flags) { return (flags >> 2) & 7; }
// where element (c, y, x) of O_o(img) lies in img [2][H][W]: img[c ^ p][v ? H-1-y : y][h ? W-1-x : x]
__device__ __forceinline__ int oriented(int o, int c, int y, int x, int H, int W) {
    return ((c ^ (o >> 2)) * H + ((o & 2) ? H - 1 - y : y)) * W + ((o & 1) ? W - 1 - x : x);
}

struct SlotInfo {
    bool active, zero;
};
__device__ __forceinline__ SlotInfo slot_info(const bmc_slot_t& e) {
    SlotInfo r;
    r.active = (e.flags & BMC_SLOT_ACTIVE) && e.frames != nullptr;
    r.zero = !r.active || (e.flags & BMC_SLOT_RESET);
    return r;
}

// grid (nbx, S), 256 threads: blockIdx.y is the slot, the blocks of a slot stride over its elements
__global__ __launch_bounds__(256) void slot_stage_kernel(const bmc_slot_t* __restrict__ table, int seqn, int H, int W,
                                                         float* __restrict__ x, const void* pool, int pool_bf16, float* feat,
                                                         int nfeat, long long feat_n, long long feat_stride, float* pred,
                                                         long long pred_n) {
    const int s = blockIdx.y;
    const bmc_slot_t e = load_slot(table, s);
    const SlotInfo si = slot_info(e);
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
    // input window: x[s][c][t][p] = frames[t][c][p] (the recording's frames i .. i+seqn-1, transposed as infer_BMCNet.py:51),
    // every frame in the slot's orientation (uniform over the slot's workgroups; code 0 takes the loop it always took)
    const int HW = H * W, o = orient_of(e.flags);
    const long long xn = 2ll * seqn * HW;
    float* const xs = x + (long long)s * xn;
    if (si.active && o) {
        for (long long i = t0; i < xn; i += step) {
            const int p = (int)(i % HW), ct = (int)(i / HW);
            const int t = ct % seqn, c = ct / seqn;
            gst<float>(xs + i, gld<float>(e.frames + (long long)t * 2 * HW + oriented(o, c, p / W, p % W, H, W)));
        }
    } else {
        for (long long i = t0; i < xn; i += step) {
            float v = 0.f;
            if (si.active) {
                const long long p = i % HW, ct = i / HW;
                const int t = (int)(ct % seqn), c = (int)(ct / seqn);
                v = gld<float>(e.frames + ((long long)t * 2 + c) * HW + p);
            }
            gst<float>(xs + i, v);
        }
    }
    // feature states: zeros, a widened bf16 pool, or a copy from a separate fp32 pool; nothing when the fp32 pool IS the buffer
    if (si.zero || pool_bf16 || (const void*)feat != pool) {
        const long long n4 = feat_n / 4;
        for (int k = 0; k < nfeat; ++k) {
            const long long o = k * feat_stride + (long long)s * feat_n;
            for (long long i = t0; i < n4; i += step) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (!si.zero) {
                    if (pool_bf16) {
                        const u16x4 b = gld<u16x4>((const unsigned short*)pool + o + 4 * i);
                        v = f32x4{bf2f(b.x), bf2f(b.y), bf2f(b.z), bf2f(b.w)};
                    } else {
                        v = gld<f32x4>((const float*)pool + o + 4 * i);
                    }
                }
                gst<f32x4>(feat + o + 4 * i, v);
            }
        }
    }
    // previous prediction (fp32, read in place by the model): zeroed where a recording starts or the slot is empty
    if (si.zero) {
        float* const ps = pred + (long long)s * pred_n;
        for (long long i = t0; i < pred_n / 4; i += step) gst<f32x4>(ps + 4 * i, f32x4{0.f, 0.f, 0.f, 0.f});
    }
}

// Self-ensemble (include/bmc_hip.h): the merge of a group's K predictions into its leader's row of the model's output, by the
// workgroups of the leader.  Lane i owns the four canonical elements 4i .. 4i+3 of [2][sH][sW]: it reads them from the leader's row
// (the identity member), hands them to the pool and to nobody else, adds the members' un-oriented values in slot order and only
// then overwrites them -- no other lane reads or writes these sixteen bytes of the leader's row, and member rows are only read.
// VEC (sW % 4 == 0): the four elements lie in one image row, a member's four sources are one aligned 16-byte load (reversed
// for a horizontal flip); otherwise four element loads.  The same additions in the same order either way.
template <bool VEC>
__device__ __forceinline__ void merge_group(const bmc_slot_t* table, int s, int K, int sH, int sW, float* pred_src,
                                            float* pred_pool, long long pred_n, float* keep, long long t0, long long step) {
    float* const lead = pred_src + (long long)s * pred_n;
    float* const pd = pred_pool + (long long)s * pred_n;
    const float scale = 1.0f / (float)K;
    for (long long i = t0; i < pred_n / 4; i += step) {
        const f32x4 own = gld<f32x4>(lead + 4 * i);
        gst<f32x4>(pd + 4 * i, own);
        f32x4 acc = own;
        const int e0 = (int)(4 * i);
        for (int j = 1; j < K; ++j) {
            const int o = orient_of(gld<int>(&table[s + j].flags));
            const float* const row = pred_src + (long long)(s + j) * pred_n;
            f32x4 u;
            if (VEC) {
                const int x0 = e0 % sW, r = e0 / sW;
                const bool h = o & 1;
                const f32x4 m = gld<f32x4>(row + oriented(o, r / sH, r % sH, h ? x0 + 3 : x0, sH, sW));
                u = h ? f32x4{m.w, m.z, m.y, m.x} : m;
            } else {
                float q[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int el = e0 + k, r = el / sW;
                    q[k] = gld<float>(row + oriented(o, r / sH, r % sH, el % sW, sH, sW));
                }
                u = f32x4{q[0], q[1], q[2], q[3]};
            }
            acc = f32x4{acc.x + u.x, acc.y + u.y, acc.z + u.z, acc.w + u.w};
        }
        const f32x4 v = {acc.x * scale, acc.y * scale, acc.z * scale, acc.w * scale};
        gst<f32x4>(lead + 4 * i, v);
        if (keep) gst<f32x4>(keep + 4 * i, v);
    }
}

struct FeatSrc {
    const float* p[3];
};

__global__ __launch_bounds__(256) void slot_commit_kernel(const bmc_slot_t* __restrict__ table, FeatSrc src, int nfeat,
                                                          long long feat_n, long long feat_stride, void* pool, int pool_bf16,
                                                          float* pred_src, float* __restrict__ pred_pool, long long pred_n) {
    const int s = blockIdx.y;
    const bmc_slot_t e = load_slot(table, s);
    if (!slot_info(e).active) return;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
    const long long n4 = feat_n / 4;
#pragma unroll
    for (int k = 0; k < 3; ++k) {           // (unrolled: the by-value pointer array is indexed by constants only -- no scratch)
        if (k >= nfeat) break;
        const float* const sp = src.p[k] + (long long)s * feat_n;
        const long long o = k * feat_stride + (long long)s * feat_n;
        for (long long i = t0; i < n4; i += step) {
            const f32x4 v = gld<f32x4>(sp + 4 * i);
            if (pool_bf16)
                gst<u16x4>((unsigned short*)pool + o + 4 * i, u16x4{f2bf(v.x), f2bf(v.y), f2bf(v.z), f2bf(v.w)});
            else
                gst<f32x4>((float*)pool + o + 4 * i, v);
        }
    }
    // the leader of an ensemble group (bits 8..11: K members from this slot on, pad_: the prediction's row length); a K or a
    // row length that does not fit the launch is no group
    const int K = (e.flags >> 8) & 15;
    if (K == 2 || K == 4 || K == 8) {
        const int sW = gld<int>(&table[s].pad_);
        if (s + K <= (int)gridDim.y && sW > 0 && pred_n < (1ll << 31) && pred_n % (2ll * sW) == 0) {
            const int sH = (int)(pred_n / (2ll * sW));
            if (sW % 4 == 0)
                merge_group<true>(table, s, K, sH, sW, pred_src, pred_pool, pred_n, e.keep, t0, step);
            else
                merge_group<false>(table, s, K, sH, sW, pred_src, pred_pool, pred_n, e.keep, t0, step);
            return;
        }
    }
    const float* const ps = pred_src + (long long)s * pred_n;
    float* const pd = pred_pool + (long long)s * pred_n;
    for (long long i = t0; i < pred_n / 4; i += step) {
        const f32x4 v = gld<f32x4>(ps + 4 * i);
        gst<f32x4>(pd + 4 * i, v);
        if (e.keep) gst<f32x4>(e.keep + 4 * i, v);
    }
}

// one output element of F.interpolate(plane [H][W] -> [Ho][Wo], 'bicubic'): the arithmetic of resize.hip's forward kernel
__device__ __forceinline__ float bicubic_at(const float* xp, int H, int W, int Y, int X, float sy, float sx) {
    int iy0, ix0;
    float wy[4], wx[4];
    cubic_taps(Y, sy, iy0, wy);
    cubic_taps(X, sx, ix0, wx);
    int cx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cx[k] = clampi(ix0 - 1 + k, 0, W - 1);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float* const row = xp + (long long)clampi(iy0 - 1 + j, 0, H - 1) * W;
        const float rv = gld<float>(row + cx[0]) * wx[0] + gld<float>(row + cx[1]) * wx[1] + gld<float>(row + cx[2]) * wx[2] +
                         gld<float>(row + cx[3]) * wx[3];
        acc += rv * wy[j];
    }
    return acc;
}

constexpr int MT = 1024;   // metrics: workgroups of 16 waves; grid (nparts, S)

__global__ __launch_bounds__(MT) void slot_metrics_kernel(const bmc_slot_t* __restrict__ table, const float* __restrict__ pred,
                                                          int sH, int sW, int H, int W, int gh, int gw, float syp, float sxp,
                                                          float syi, float sxi) {
    __shared__ double red[2][MT];
    const int part = blockIdx.x, nparts = gridDim.x, s = blockIdx.y, tid = threadIdx.x;
    const bmc_slot_t e = load_slot(table, s);
    if (!slot_info(e).active || e.result == nullptr) return;       // (uniform over the workgroup)
    const float* const ps = pred + (long long)s * 2 * sH * sW;
    const float* const in = e.frames + 2ll * H * W;               // inp_cnt[:, 1]: frame 1 of the window
    const bool same = sH == gh && sW == gw;
    const int n = 2 * gh * gw;
    double ae = 0.0, ab = 0.0;
    for (int i = part * MT + tid; i < n; i += nparts * MT) {      // part p owns a fixed set of elements
        const int X = i % gw, r = i / gw, Y = r % gh, c = r / gh;
        const float g = gld<float>(e.gt + i);
        const float pv = same ? gld<float>(ps + i) : bicubic_at(ps + (long long)c * sH * sW, sH, sW, Y, X, syp, sxp);
        const float bv = bicubic_at(in + (long long)c * H * W, H, W, Y, X, syi, sxi);
        const float de = pv - g, db = bv - g;
        ae += (double)(de * de);
        ab += (double)(db * db);
    }
    red[0][tid] = ae;
    red[1][tid] = ab;
    __syncthreads();
    for (int w = MT / 2; w > 0; w >>= 1) {                         // fixed tree: the same sums in the same order every run
        if (tid < w) {
            red[0][tid] += red[0][tid + w];
            red[1][tid] += red[1][tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        gst<double>(e.result + 2 * part, red[0][0]);
        gst<double>(e.result + 2 * part + 1, red[1][0]);
    }
}

inline int slot_blocks(long long per_slot, int S) {
    const long long cap = S >= 64 ? 16 : 1024 / S;
    long long b = (per_slot + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
inline bool al16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

}  // namespace

extern "C" int bmc_slot_stage(const bmc_slot_t* table, int S, int seqn, int H, int W, float* x, const void* feat_pool,
                              int pool_bf16, float* feat, int nfeat, long long feat_n, float* pred, long long pred_n,
                              bmc_stream_t s) {
    BMC_CHECK_ARG(table && x && feat_pool && feat && pred && S >= 1 && S <= BMC_MAX_SLOTS && seqn >= 2 && H > 0 && W > 0 &&
                      nfeat >= 1 && nfeat <= 3 && feat_n > 0 && feat_n % 4 == 0 && pred_n > 0 && pred_n % 4 == 0,
                  "bmc_slot_stage: bad arguments");
    BMC_CHECK_ARG(al16(feat) && al16(pred) && (pool_bf16 ? ((unsigned long long)feat_pool & 7ull) == 0 : al16(feat_pool)),
                  "bmc_slot_stage: state buffers must be 16-byte aligned (8 for a bf16 pool)");
    BMC_CHECK_ARG(!(pool_bf16 && (const void*)feat == feat_pool), "bmc_slot_stage: a bf16 pool cannot be the fp32 buffer");
    long long work = feat_n / 4;
    if (2ll * seqn * H * W > work) work = 2ll * seqn * H * W;
    if (pred_n / 4 > work) work = pred_n / 4;
    hipLaunchKernelGGL(slot_stage_kernel, dim3(slot_blocks(work, S), S), dim3(256), 0, (hipStream_t)s, table, seqn, H, W, x,
                       feat_pool, pool_bf16, feat, nfeat, feat_n, (long long)S * feat_n, pred, pred_n);
    BMC_CHECK_LAUNCH("bmc_slot_stage");
    return 0;
}

extern "C" int bmc_slot_commit(const bmc_slot_t* table, int S, const float* const* feat_src, int nfeat, long long feat_n,
                               void* feat_pool, int pool_bf16, float* pred_src, float* pred_pool, long long pred_n,
                               bmc_stream_t s) {
    BMC_CHECK_ARG(table && feat_src && feat_pool && pred_src && pred_pool && S >= 1 && S <= BMC_MAX_SLOTS && nfeat >= 1 &&
                      nfeat <= 3 && feat_n > 0 && feat_n % 4 == 0 && pred_n > 0 && pred_n % 4 == 0,
                  "bmc_slot_commit: bad arguments");
    FeatSrc fs = {{nullptr, nullptr, nullptr}};
    for (int k = 0; k < nfeat; ++k) {
        BMC_CHECK_ARG(feat_src[k] && al16(feat_src[k]), "bmc_slot_commit: feature source %d null or not 16-byte aligned", k);
        fs.p[k] = feat_src[k];
    }
    BMC_CHECK_ARG(al16(pred_src) && al16(pred_pool) && (pool_bf16 ? ((unsigned long long)feat_pool & 7ull) == 0 : al16(feat_pool)),
                  "bmc_slot_commit: state buffers must be 16-byte aligned (8 for a bf16 pool)");
    const long long work = feat_n / 4 > pred_n / 4 ? feat_n / 4 : pred_n / 4;
    hipLaunchKernelGGL(slot_commit_kernel, dim3(slot_blocks(work, S), S), dim3(256), 0, (hipStream_t)s, table, fs, nfeat, feat_n,
                       (long long)S * feat_n, feat_pool, pool_bf16, pred_src, pred_pool, pred_n);
    BMC_CHECK_LAUNCH("bmc_slot_commit");
    return 0;
}

extern "C" int bmc_slot_metrics(const bmc_slot_t* table, int S, const float* pred, int sH, int sW, int H, int W, int gh, int gw,
                                int nparts, bmc_stream_t s) {
    BMC_CHECK_ARG(table && pred && S >= 1 && S <= BMC_MAX_SLOTS && sH > 0 && sW > 0 && H > 0 && W > 0 && gh > 0 && gw > 0 &&
                      2ll * gh * gw < (1ll << 30) && nparts >= 1 && nparts <= BMC_SLOT_MAX_PARTS,
                  "bmc_slot_metrics: bad arguments");
    hipLaunchKernelGGL(slot_metrics_kernel, dim3(nparts, S), dim3(MT), 0, (hipStream_t)s, table, pred, sH, sW, H, W, gh, gw,
                       (float)sH / (float)gh, (float)sW / (float)gw, (float)H / (float)gh, (float)W / (float)gw);
    BMC_CHECK_LAUNCH("bmc_slot_metrics");
    return 0;
}
