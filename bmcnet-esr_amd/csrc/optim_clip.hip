// The clipped optimizer step (bmcnet-esr_amd/bmc_hip/optim.py::Adam(max_grad_norm=, nonfinite=)): clipping by the global gradient
// norm and the skip of a step whose gradients are not finite, without a host round trip.  The contract is stated once in
// include/bmc_hip.h "optimizer step: clipping".
//
// Two launches over the chunk table of optim.hip.  grad_sq_kernel reads g alone (4 bytes per element) and stores one float64 partial
// per chunk, the bits adam_kernel<.., NORM = true, ..> stores.  clip_step_kernel is the pass of optim.hip (36 bytes per element) in
// which every workgroup first adds ALL partials of the step in one fixed order, so that all hold the same coefficient c, and then
// runs adam_elem (adam_k.h, the function optim.hip compiles) on g * c.  Global accesses only, no scratch, no atomics, no
// workgroup waits for another.
#include "adam_k.h"

namespace {

// ---- the norm launch: lane-to-element assignment, per-lane order and tree of adam_kernel<.., NORM = true, ..>
__global__ __launch_bounds__(AT) void grad_sq_kernel(const bmc_adam_chunk_t* __restrict__ table, double* __restrict__ partial_sq) {
    __shared__ double red[AT];
    const int tid = threadIdx.x;
    const bmc_adam_chunk_t* const ent = table + blockIdx.x;
    const float* const g = uniform_ptr<const float>(&ent->g);
    int n = __builtin_amdgcn_readfirstlane(gld<int>(&ent->n));
    n = n < BMC_ADAM_CHUNK ? n : BMC_ADAM_CHUNK;
    const bool aligned = __builtin_amdgcn_readfirstlane(gld<int>(&ent->aligned)) != 0;
    double acc = 0.0;
    if (aligned) {
        const int nvec = n >> 2;
        f32x4 G[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j)
            if (tid + j * AT < nvec) G[j] = gld<f32x4>(g + 4 * (tid + j * AT));
#pragma unroll
        for (int j = 0; j < VPL; ++j)
            if (tid + j * AT < nvec) {
#pragma unroll
                for (int c = 0; c < 4; ++c) acc += sq(G[j][c]);
            }
        const int e = 4 * nvec + tid;              // the last partial vector, one element per lane
        if (e < n) acc += sq(gld<float>(g + e));
    } else {
        for (int e = tid; e < n; e += AT) acc += sq(gld<float>(g + e));
    }
    const double total = tree_sum(red, acc, tid);
    if (tid == 0) gst<double>(partial_sq + blockIdx.x, total);
}

// ---- the coefficient: float32, one rounding per line (torch.nn.utils.clip_grad_norm_: max_norm / (norm + 1e-6), clamped at 1)
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

template <bool AMS, bool FULL>
__device__ __forceinline__ void vec_load(const float* p, const float* g, const float* m, const float* v, const float* x, int nvec,
                                         int tid, f32x4* P, f32x4* G, f32x4* M, f32x4* V, f32x4* X) {
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int e = 4 * (tid + j * AT);
        if (FULL || tid + j * AT < nvec) {
            P[j] = gld<f32x4>(p + e); G[j] = gld<f32x4>(g + e); M[j] = gld<f32x4>(m + e); V[j] = gld<f32x4>(v + e);
            if constexpr (AMS) X[j] = gld<f32x4>(x + e);
        }
    }
}

template <bool AMS, bool FULL>
__device__ __forceinline__ void vec_apply(float* p, float* m, float* v, float* x, int nvec, int tid, const AdamK& k, float c,
                                          f32x4* P, f32x4* G, f32x4* M, f32x4* V, f32x4* X) {
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int e = 4 * (tid + j * AT);
        if (FULL || tid + j * AT < nvec) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float pe = P[j][i], me = M[j][i], ve = V[j][i], xe = AMS ? X[j][i] : 0.f;
                adam_elem<AMS>(pe, clip_g(G[j][i], c), me, ve, xe, k);
                P[j][i] = pe; M[j][i] = me; V[j][i] = ve;
                if constexpr (AMS) X[j][i] = xe;
            }
            gst<f32x4>(p + e, P[j]); gst<f32x4>(m + e, M[j]); gst<f32x4>(v + e, V[j]);
            if constexpr (AMS) gst<f32x4>(x + e, X[j]);
        }
    }
}

// grid: n_chunks workgroups.  AMS: amsgrad; CAP: the step count comes from *step_dev.
template <bool AMS, bool CAP>
__global__ __launch_bounds__(AT) void clip_step_kernel(const bmc_adam_chunk_t* __restrict__ table, const bmc_adam_hyper_t h,
                                                       const int* __restrict__ step_dev, const bmc_adam_clip_t clip) {
    __shared__ double red[AT];
    const int tid = threadIdx.x;
    const bmc_adam_chunk_t* const ent = table + blockIdx.x;
    float* const p = uniform_ptr<float>(&ent->p);
    const float* const g = uniform_ptr<const float>(&ent->g);
    float* const m = uniform_ptr<float>(&ent->m);
    float* const v = uniform_ptr<float>(&ent->v);
    float* const x = AMS ? uniform_ptr<float>(&ent->vmax) : nullptr;
    int n = __builtin_amdgcn_readfirstlane(gld<int>(&ent->n));
    n = n < BMC_ADAM_CHUNK ? n : BMC_ADAM_CHUNK;
    const bool aligned = __builtin_amdgcn_readfirstlane(gld<int>(&ent->aligned)) != 0;
    const bool full = aligned && n == BMC_ADAM_CHUNK;

    // the total of ALL partials of the step, the same bits in every workgroup: lane t adds partial t, t + 256, ... in that order
    double acc = 0.0;
    for (int i = tid; i < clip.n_partials; i += AT) acc += gld<double>(clip.partial_sq + i);
    const double total = tree_sum(red, acc, tid);
    const double norm = __builtin_sqrt(total);
    const float c = clip_coeff(norm, clip.max_norm);
    const bool skip = clip.skip_nonfinite != 0 && !__builtin_isfinite(total);      // uniform over the whole grid
    if (blockIdx.x == 0 && tid == 0) {             // plain stores by one lane
        if (clip.info) { gst<double>(clip.info, norm); gst<double>(clip.info + 1, (double)c); }
        if (skip && clip.skipped) gst<int>(clip.skipped, gld<int>(clip.skipped) + 1);
    }
    if (skip) return;                              // nothing of p, m, v, vmax is stored

    AdamK k;
    k.omb1 = h.one_minus_beta1; k.beta2 = h.beta2; k.omb2 = h.one_minus_beta2; k.eps = h.eps; k.wd = h.weight_decay;
    if constexpr (CAP) {
        __shared__ float sh[2];
        if (tid == 0) {                            // float64, once per workgroup, as the host does for the plain entry point
            const double t = (double)(gld<int>(step_dev) + 1);
            sh[0] = (float)(h.lr / (1.0 - pow(h.beta1_f64, t)));
            sh[1] = (float)sqrt(1.0 - pow(h.beta2_f64, t));
        }
        __syncthreads();
        k.step_size = sh[0]; k.bc2s = sh[1];
    } else {
        k.step_size = h.step_size; k.bc2s = h.bias_correction2_sqrt;
    }

    // The partials are reduced BEFORE the chunk's loads are issued.  Issuing a full chunk's 20 loads first, so that the reduction
    // runs under their latency, was measured and is slower: the 80 registers held across the reduction cost the kernel its
    // occupancy (248 against 194 VGPRs), 24.6 against 17.6 us for the BMCNet(4,128,5) set on an MI355X.
    f32x4 P[VPL], G[VPL], M[VPL], V[VPL], X[VPL];
    if (full) {
        vec_load<AMS, true>(p, g, m, v, x, VPL * AT, tid, P, G, M, V, X);
        vec_apply<AMS, true>(p, m, v, x, VPL * AT, tid, k, c, P, G, M, V, X);
    } else if (aligned) {
        const int nvec = n >> 2;
        vec_load<AMS, false>(p, g, m, v, x, nvec, tid, P, G, M, V, X);
        vec_apply<AMS, false>(p, m, v, x, nvec, tid, k, c, P, G, M, V, X);
        const int e = 4 * nvec + tid;              // the last partial vector, one element per lane
        if (e < n) {
            const float ge = clip_g(gld<float>(g + e), c);
            float pe = gld<float>(p + e), me = gld<float>(m + e), ve = gld<float>(v + e), xe = AMS ? gld<float>(x + e) : 0.f;
            adam_elem<AMS>(pe, ge, me, ve, xe, k);
            gst<float>(p + e, pe); gst<float>(m + e, me); gst<float>(v + e, ve);
            if constexpr (AMS) gst<float>(x + e, xe);
        }
    } else {
        for (int e = tid; e < n; e += AT) {
            const float ge = clip_g(gld<float>(g + e), c);
            float pe = gld<float>(p + e), me = gld<float>(m + e), ve = gld<float>(v + e), xe = AMS ? gld<float>(x + e) : 0.f;
            adam_elem<AMS>(pe, ge, me, ve, xe, k);
            gst<float>(p + e, pe); gst<float>(m + e, me); gst<float>(v + e, ve);
            if constexpr (AMS) gst<float>(x + e, xe);
        }
    }
}

// the last launch of the capturable entry point: one lane, a plain vector store (also after a skipped step)
__global__ void clip_advance_kernel(int* __restrict__ step_dev) {
    if (threadIdx.x == 0) gst<int>(step_dev, gld<int>(step_dev) + 1);
}

int clip_check(const char* name, int n_chunks, const bmc_adam_clip_t& clip) {
    BMC_CHECK_ARG(clip.partial_sq || n_chunks == 0, "%s: no partial_sq (the norm launches of the step write it)", name);
    BMC_CHECK_ARG(clip.n_partials >= n_chunks, "%s: n_partials = %d is less than n_chunks = %d", name, clip.n_partials, n_chunks);
    BMC_CHECK_ARG(clip.max_norm > 0.f, "%s: max_norm = %g is not a positive number (+INF: never clip)", name, clip.max_norm);
    BMC_CHECK_ARG(clip.skip_nonfinite == 0 || clip.skip_nonfinite == 1, "%s: skip_nonfinite = %d is neither 0 nor 1", name,
                  clip.skip_nonfinite);
    return 0;
}

}  // namespace

extern "C" int bmc_adam_grad_sq(const bmc_adam_chunk_t* table, int n_chunks, double* partial_sq, bmc_stream_t s) {
    BMC_CHECK_ARG(n_chunks >= 0, "bmc_adam_grad_sq: n_chunks = %d is negative", n_chunks);
    BMC_CHECK_ARG(table || n_chunks == 0, "bmc_adam_grad_sq: no chunk table for %d chunks", n_chunks);
    BMC_CHECK_ARG(partial_sq || n_chunks == 0, "bmc_adam_grad_sq: no partial_sq for %d chunks", n_chunks);
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(grad_sq_kernel, dim3((unsigned)n_chunks), dim3(AT), 0, (hipStream_t)s, table, partial_sq);
    BMC_CHECK_LAUNCH("bmc_adam_grad_sq");
    return 0;
}

extern "C" int bmc_adam_step_clipped(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, bmc_adam_clip_t clip,
                                     bmc_stream_t s) {
    if (adam_check("bmc_adam_step_clipped", table, n_chunks, hyper, false)) return -1;
    if (clip_check("bmc_adam_step_clipped", n_chunks, clip)) return -1;
    if (n_chunks == 0) return 0;
    const auto fn = hyper.amsgrad != 0 ? clip_step_kernel<true, false> : clip_step_kernel<false, false>;
    hipLaunchKernelGGL(fn, dim3((unsigned)n_chunks), dim3(AT), 0, (hipStream_t)s, table, hyper, (const int*)nullptr, clip);
    BMC_CHECK_LAUNCH("bmc_adam_step_clipped");
    return 0;
}

extern "C" int bmc_adam_step_clipped_capturable(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, int* step_dev,
                                                bmc_adam_clip_t clip, bmc_stream_t s) {
    if (adam_check("bmc_adam_step_clipped_capturable", table, n_chunks, hyper, true)) return -1;
    if (clip_check("bmc_adam_step_clipped_capturable", n_chunks, clip)) return -1;
    BMC_CHECK_ARG(step_dev || n_chunks == 0, "bmc_adam_step_clipped_capturable: no step counter");
    if (n_chunks == 0) return 0;
    const auto fn = hyper.amsgrad != 0 ? clip_step_kernel<true, true> : clip_step_kernel<false, true>;
    hipLaunchKernelGGL(fn, dim3((unsigned)n_chunks), dim3(AT), 0, (hipStream_t)s, table, hyper, (const int*)step_dev, clip);
    BMC_CHECK_LAUNCH("bmc_adam_step_clipped_capturable");
    hipLaunchKernelGGL(clip_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, step_dev);
    BMC_CHECK_LAUNCH("bmc_adam_step_clipped_capturable");
    return 0;
}
