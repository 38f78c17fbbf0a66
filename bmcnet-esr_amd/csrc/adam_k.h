// The device pieces of the optimizer step, each written once: the element arithmetic, the view of a chunk, the walk over it (with
// and without the state tensors), the set-up of the step's constants, the body of the unclipped step and the head of the clipped
// one.  Every kernel of the family rounds alike because it runs THIS adam_elem over THIS walk.  Two translation units compile it:
// optim.hip, whose kernels are the EMA = false instantiations, and optim_ema.hip, whose kernels are the EMA = true ones and the
// exchange of weights and averages.  (Two, because tests/optim_asm.py pins optim.hip's kernel count and mangled names.)  Internal;
// the contracts are include/bmc_hip.h "optimizer step" and include/bmc_hip_ema.h.
#pragma once
#include <math.h>
#include "bmc_common.h"
#include "bmc_hip_ema.h"
#include "slot_k.h"

// ---- host: the argument checks and the advance launch of the entry points, defined in optim.hip for both translation units
namespace bmc_adam_host {
int adam_check(const char* name, const bmc_adam_chunk_t* table, int n_chunks, const bmc_adam_hyper_t& h, bool cap);
int clip_check(const char* name, int n_chunks, const bmc_adam_clip_t& clip);
int advance(const char* name, int* step_dev, bmc_stream_t s);      // the second launch of every capturable entry point
}

namespace {

constexpr int AT = 256;                            // lanes per workgroup
constexpr int VPL = BMC_ADAM_CHUNK / 4 / AT;       // 16-byte vectors per lane of a full chunk
static_assert(VPL * 4 * AT == BMC_ADAM_CHUNK, "a full chunk is a whole number of rounds of the workgroup");

struct AdamK {
    float omb1, beta2, omb2, eps, wd, step_size, bc2s;
    float w;                                       // EMA: (float)(1 - decay_t), otherwise not set
};

// One element.  Every load path calls this, so they round alike.  sqrt and the divisions are the compiler's own operators: in a HIP
// compile these are the correctly rounded ones (the __fsqrt_rn / __fdiv_rn spellings are NOT: without OCML's rounded-operations
// switch __fsqrt_rn is the native, 1-ulp square root).
template <bool AMS>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float& vmax, const AdamK& k) {
#pragma clang fp contract(off)      // the rounding points are the ones written here, whatever the compiler prefers
    if (k.wd != 0.f) g = g + k.wd * p;
    m = m + k.omb1 * (g - m);
    v = v * k.beta2 + k.omb2 * (g * g);
    float d = v;
    if constexpr (AMS) {
        const float r = v > vmax ? v : vmax;       // a NaN vmax stays (the comparison is false) ...
        vmax = v != v ? v : r;                     // ... and a NaN v wins: torch.maximum
        d = vmax;
    }
    const float den = __builtin_sqrtf(d) / k.bc2s + k.eps;
    p = p - k.step_size * (m / den);
}

// The moving average of one element, after adam_elem has made the new p: three roundings (include/bmc_hip_ema.h).
__device__ __forceinline__ void ema_elem(float& e, float p, float w) {
#pragma clang fp contract(off)
    const float d = p - e;
    const float s = w * d;
    e = e + s;
}

template <class T>
__device__ __forceinline__ T* uniform_ptr(const void* slot) {      // a table pointer, the same for every lane -> scalar registers
    const unsigned long long v = gld<unsigned long long>(slot);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ double sq(float g) { return (double)g * (double)g; }

// The fixed tree over the workgroup's 256 float64 values: every lane returns the same bits.  red: AT doubles of LDS.
__device__ __forceinline__ double tree_sum(double* red, double acc, int tid) {
    red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int s = AT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// ---- the coefficient of a clipped step: float32, one rounding per line (torch.nn.utils.clip_grad_norm_: max_norm / (norm + 1e-6),
// clamped at 1)
__device__ __forceinline__ float clip_coeff(double norm, float max_norm) {
#pragma clang fp contract(off)
    const float n32 = (float)norm;
    const float s = n32 + 1e-6f;
    const float q = max_norm / s;
    return q > 1.0f ? 1.0f : q;                    // a NaN q stays NaN: torch.clamp(max=1.0)
}

__device__ __forceinline__ float clip_g(float g, float c) {
#pragma clang fp contract(off)      // g * c is a rounding of its own; it never fuses into the first line of adam_elem
    return g * c;
}

// ---- what a step does to every g before adam_elem sees it
struct GradAsIs {                                  // the plain step
    __device__ __forceinline__ float operator()(float g) const { return g; }
};
struct GradSumSq {                                 // ... that also adds the RAW g to this lane's share of sum(g^2)
    double& acc;
    __device__ __forceinline__ float operator()(float g) const { acc += sq(g); return g; }
};
struct GradClipped {                               // the clipped step
    float c;
    __device__ __forceinline__ float operator()(float g) const { return clip_g(g, c); }
};

// ---- one workgroup's chunk: the table's pointers made wave-uniform, n clamped to what a workgroup covers
struct Chunk {
    float* p;
    const float* g;
    float *m, *v, *x;                              // x: vmax, nullptr without amsgrad
    int n;
    bool aligned;
    float* e;                                      // EMA: the chunk's average, at the element offset of p; otherwise not set
};

template <bool AMS>
__device__ __forceinline__ Chunk chunk_view(const bmc_adam_chunk_t* ent) {
    Chunk ck;
    ck.p = uniform_ptr<float>(&ent->p);
    ck.g = uniform_ptr<const float>(&ent->g);
    ck.m = uniform_ptr<float>(&ent->m);
    ck.v = uniform_ptr<float>(&ent->v);
    ck.x = AMS ? uniform_ptr<float>(&ent->vmax) : nullptr;
    const int n = __builtin_amdgcn_readfirstlane(gld<int>(&ent->n));
    ck.n = n < BMC_ADAM_CHUNK ? n : BMC_ADAM_CHUNK;
    ck.aligned = __builtin_amdgcn_readfirstlane(gld<int>(&ent->aligned)) != 0;
    ck.e = nullptr;
    return ck;
}

// element e on its own: the tail of an aligned chunk and every element of an unaligned one
template <bool AMS, bool EMA, class Grad>
__device__ __forceinline__ void step_elem(const Chunk& ck, int e, const AdamK& k, const Grad& grad) {
    const float ge = grad(gld<float>(ck.g + e));
    float pe = gld<float>(ck.p + e), me = gld<float>(ck.m + e), ve = gld<float>(ck.v + e), xe = AMS ? gld<float>(ck.x + e) : 0.f;
    float ee = EMA ? gld<float>(ck.e + e) : 0.f;
    adam_elem<AMS>(pe, ge, me, ve, xe, k);
    if constexpr (EMA) ema_elem(ee, pe, k.w);
    gst<float>(ck.p + e, pe); gst<float>(ck.m + e, me); gst<float>(ck.v + e, ve);
    if constexpr (AMS) gst<float>(ck.x + e, xe);
    if constexpr (EMA) gst<float>(ck.e + e, ee);
}

// The whole 16-byte vectors of an aligned chunk: vector tid + j * AT is this lane's j-th.  FULL: the chunk has all 4096 elements and
// nothing is guarded -- straight-line code, the 20 loads of a lane (24 with EMA) are issued before the first is used.
template <bool AMS, bool FULL, bool EMA, class Grad>
__device__ __forceinline__ void vec_pass(const Chunk& ck, int nvec, int tid, const AdamK& k, const Grad& grad) {
    f32x4 P[VPL], G[VPL], M[VPL], V[VPL], X[VPL], E[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int e = 4 * (tid + j * AT);
        if (FULL || tid + j * AT < nvec) {
            P[j] = gld<f32x4>(ck.p + e); G[j] = gld<f32x4>(ck.g + e); M[j] = gld<f32x4>(ck.m + e); V[j] = gld<f32x4>(ck.v + e);
            if constexpr (AMS) X[j] = gld<f32x4>(ck.x + e);
            if constexpr (EMA) E[j] = gld<f32x4>(ck.e + e);
        }
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int e = 4 * (tid + j * AT);
        if (FULL || tid + j * AT < nvec) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float pe = P[j][c], me = M[j][c], ve = V[j][c], xe = AMS ? X[j][c] : 0.f;
                adam_elem<AMS>(pe, grad(G[j][c]), me, ve, xe, k);
                P[j][c] = pe; M[j][c] = me; V[j][c] = ve;
                if constexpr (AMS) X[j][c] = xe;
                if constexpr (EMA) { float ee = E[j][c]; ema_elem(ee, pe, k.w); E[j][c] = ee; }
            }
            gst<f32x4>(ck.p + e, P[j]); gst<f32x4>(ck.m + e, M[j]); gst<f32x4>(ck.v + e, V[j]);
            if constexpr (AMS) gst<f32x4>(ck.x + e, X[j]);
            if constexpr (EMA) gst<f32x4>(ck.e + e, E[j]);
        }
    }
}

// ---- THE WALK.  step_chunk and grad_sq_chunk give a lane the same elements in the same order, which is why the partials of the norm
// launch are the bits a step launch with GradSumSq stores.  Aligned chunk: the lane's vectors tid + j * AT for j = 0 .. VPL - 1 below
// n / 4, components 0 .. 3 of each, then element 4 * (n / 4) + tid of the last partial vector.  Unaligned chunk: elements tid,
// tid + AT, ... below n.  Change one of the two functions and the other changes with it.
template <bool AMS, bool EMA, class Grad>
__device__ __forceinline__ void step_chunk(const Chunk& ck, int tid, const AdamK& k, const Grad& grad) {
    if (ck.aligned) {
        const int nvec = ck.n >> 2;
        if (ck.n == BMC_ADAM_CHUNK) vec_pass<AMS, true, EMA>(ck, nvec, tid, k, grad);      // all loads in flight, then the arithmetic
        else vec_pass<AMS, false, EMA>(ck, nvec, tid, k, grad);
        const int e = 4 * nvec + tid;
        if (e < ck.n) step_elem<AMS, EMA>(ck, e, k, grad);
    } else {
        for (int e = tid; e < ck.n; e += AT) step_elem<AMS, EMA>(ck, e, k, grad);
    }
}

// the same walk over p and e alone: the two exchanged, bit for bit
__device__ __forceinline__ void swap_chunk(const Chunk& ck, int tid) {
    auto one = [&](int e) {
        const float pe = gld<float>(ck.p + e), ee = gld<float>(ck.e + e);
        gst<float>(ck.p + e, ee); gst<float>(ck.e + e, pe);
    };
    if (ck.aligned) {
        const int nvec = ck.n >> 2;
        f32x4 P[VPL], E[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j)
            if (tid + j * AT < nvec) { P[j] = gld<f32x4>(ck.p + 4 * (tid + j * AT)); E[j] = gld<f32x4>(ck.e + 4 * (tid + j * AT)); }
#pragma unroll
        for (int j = 0; j < VPL; ++j)
            if (tid + j * AT < nvec) { gst<f32x4>(ck.p + 4 * (tid + j * AT), E[j]); gst<f32x4>(ck.e + 4 * (tid + j * AT), P[j]); }
        const int e = 4 * nvec + tid;
        if (e < ck.n) one(e);
    } else {
        for (int e = tid; e < ck.n; e += AT) one(e);
    }
}

// the same walk over g alone -> this lane's share of sum(g^2)
__device__ __forceinline__ double grad_sq_chunk(const Chunk& ck, int tid) {
    double acc = 0.0;
    if (ck.aligned) {
        const int nvec = ck.n >> 2;
        f32x4 G[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j)
            if (tid + j * AT < nvec) G[j] = gld<f32x4>(ck.g + 4 * (tid + j * AT));
#pragma unroll
        for (int j = 0; j < VPL; ++j)
            if (tid + j * AT < nvec) {
#pragma unroll
                for (int c = 0; c < 4; ++c) acc += sq(G[j][c]);
            }
        const int e = 4 * nvec + tid;
        if (e < ck.n) acc += sq(gld<float>(ck.g + e));
    } else {
        for (int e = tid; e < ck.n; e += AT) acc += sq(gld<float>(ck.g + e));
    }
    return acc;
}

// ---- the constants of a step.  CAP: the step count comes from *step_dev and the two bias corrections are computed here, in float64,
// once per workgroup, as the host does for the plain entry points (every lane of the workgroup must call this: it holds a barrier).
// EMA: the same lane computes w = (float)(1 - decay_t) from the same t, a skipped step counted (include/bmc_hip_ema.h).
struct NoEma {};
template <bool CAP, bool EMA, class Ema>
__device__ __forceinline__ AdamK adam_setup(const bmc_adam_hyper_t& h, const int* step_dev, int tid, const Ema& ema) {
    AdamK k;
    k.omb1 = h.one_minus_beta1; k.beta2 = h.beta2; k.omb2 = h.one_minus_beta2; k.eps = h.eps; k.wd = h.weight_decay;
    k.w = 0.f;
    if constexpr (CAP) {
        __shared__ float sh[EMA ? 3 : 2];
        if (tid == 0) {
            const double t = (double)(gld<int>(step_dev) + 1);
            sh[0] = (float)(h.lr / (1.0 - pow(h.beta1_f64, t)));
            sh[1] = (float)sqrt(1.0 - pow(h.beta2_f64, t));
            if constexpr (EMA) {
                double decay_t = ema.decay;
                if (ema.warmup != 0) {
                    const double ramp = t / (t + 9.0);
                    decay_t = ramp < decay_t ? ramp : decay_t;
                }
                sh[2] = (float)(1.0 - decay_t);
            }
        }
        __syncthreads();
        k.step_size = sh[0]; k.bc2s = sh[1];
        if constexpr (EMA) k.w = sh[2];
    } else {
        k.step_size = h.step_size; k.bc2s = h.bias_correction2_sqrt;
        if constexpr (EMA) k.w = ema.w;
    }
    return k;
}

// ---- the body of the unclipped step kernels.  grid: n_chunks workgroups of AT lanes.  AMS: amsgrad; NORM: partial_sq is given; CAP:
// the step count comes from *step_dev; EMA: ema is a bmc_adam_ema_t and every element's average moves with it (otherwise NoEma).
template <bool AMS, bool NORM, bool CAP, bool EMA, class Ema>
__device__ __forceinline__ void adam_body(const bmc_adam_chunk_t* table, const bmc_adam_hyper_t& h, const int* step_dev,
                                          double* partial_sq, const Ema& ema) {
    const int tid = threadIdx.x;
    Chunk ck = chunk_view<AMS>(table + blockIdx.x);
    if constexpr (EMA) ck.e = uniform_ptr<float>(ema.e + blockIdx.x);
    const AdamK k = adam_setup<CAP, EMA>(h, step_dev, tid, ema);
    if constexpr (NORM) {
        __shared__ double red[AT];
        double acc = 0.0;                          // this lane's share of sum(g^2), added in index order
        step_chunk<AMS, EMA>(ck, tid, k, GradSumSq{acc});
        const double total = tree_sum(red, acc, tid);
        if (tid == 0) gst<double>(partial_sq + blockIdx.x, total);
    } else {
        step_chunk<AMS, EMA>(ck, tid, k, GradAsIs{});
    }
}

// The head of a clipped step, the text of both clipped kernels (a macro, not a function: the `return` is the kernel's own, and the
// compiler keeps `skip` in scalar registers as it does when the lines stand in the kernel).  It defines c, the coefficient, and
// returns from the kernel when the step is skipped -- uniformly over the whole grid, before anything of p, m, v, vmax or e is loaded
// or stored.  red: AT doubles of LDS.
#define BMC_CLIP_STEP_HEAD(clip, red, tid)                                                                                          \
    /* the total of ALL partials of the step, the same bits in every workgroup: lane t adds partial t, t + 256, ... in that order */ \
    double acc = 0.0;                                                                                                               \
    for (int i = tid; i < clip.n_partials; i += AT) acc += gld<double>(clip.partial_sq + i);                                        \
    const double total = tree_sum(red, acc, tid);                                                                                   \
    const double norm = __builtin_sqrt(total);                                                                                      \
    const float c = clip_coeff(norm, clip.max_norm);                                                                                \
    const bool skip = clip.skip_nonfinite != 0 && !__builtin_isfinite(total);      /* uniform over the whole grid */                \
    if (blockIdx.x == 0 && tid == 0) {             /* plain stores by one lane */                                                   \
        if (clip.info) { gst<double>(clip.info, norm); gst<double>(clip.info + 1, (double)c); }                                     \
        if (skip && clip.skipped) gst<int>(clip.skipped, gld<int>(clip.skipped) + 1);                                               \
    }                                                                                                                               \
    if (skip) return

}  // namespace
