// Optimizer step (bmcnet-esr_amd/bmc_hip/optim.py::Adam): torch.optim.Adam(amsgrad, weight_decay) for every parameter of a group in
// ONE launch over a device table of chunks.  The contract -- the six roundings per element, the chunk table, the gradient-norm
// partials, the capturable variant -- is stated once in include/bmc_hip.h "optimizer step".
//
// An HBM-bound element-wise pass: 36 bytes per element (read p, g, m, v, vmax; write p, m, v, vmax), each touched once.  A
// workgroup of 256 lanes owns one chunk of at most 4096 elements of one tensor: a lane issues its (up to) 20 16-byte loads, then
// computes, then stores.  The table's pointers are made wave-uniform (readfirstlane) and every access goes through the
// address-space(1) accessors of slot_k.h: scalar base + lane offset, global_* instructions, never flat_*.  No workgroup waits for
// another, no atomics, no scratch memory.
#include "adam_k.h"                            // AT, VPL, AdamK, adam_elem, uniform_ptr, sq, tree_sum, adam_check

namespace {

// The whole 16-byte vectors of an aligned chunk: vector tid + j * AT is this lane's j-th.  FULL: the chunk has all 4096 elements and
// nothing is guarded -- straight-line code, the 20 loads of a lane are issued before the first is used.
template <bool AMS, bool NORM, bool FULL>
__device__ __forceinline__ void vec_pass(float* p, const float* g, float* m, float* v, float* x, int nvec, int tid, const AdamK& k,
                                         double& acc) {
    f32x4 P[VPL], G[VPL], M[VPL], V[VPL], X[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int e = 4 * (tid + j * AT);
        if (FULL || tid + j * AT < nvec) {
            P[j] = gld<f32x4>(p + e); G[j] = gld<f32x4>(g + e); M[j] = gld<f32x4>(m + e); V[j] = gld<f32x4>(v + e);
            if constexpr (AMS) X[j] = gld<f32x4>(x + e);
        }
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int e = 4 * (tid + j * AT);
        if (FULL || tid + j * AT < nvec) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if constexpr (NORM) acc += sq(G[j][c]);
                float pe = P[j][c], me = M[j][c], ve = V[j][c], xe = AMS ? X[j][c] : 0.f;
                adam_elem<AMS>(pe, G[j][c], me, ve, xe, k);
                P[j][c] = pe; M[j][c] = me; V[j][c] = ve;
                if constexpr (AMS) X[j][c] = xe;
            }
            gst<f32x4>(p + e, P[j]); gst<f32x4>(m + e, M[j]); gst<f32x4>(v + e, V[j]);
            if constexpr (AMS) gst<f32x4>(x + e, X[j]);
        }
    }
}

// grid: n_chunks workgroups.  AMS: amsgrad; NORM: partial_sq is given; CAP: the step count comes from *step_dev.
template <bool AMS, bool NORM, bool CAP>
__global__ __launch_bounds__(AT) void adam_kernel(const bmc_adam_chunk_t* __restrict__ table, const bmc_adam_hyper_t h,
                                                  const int* __restrict__ step_dev, double* __restrict__ partial_sq) {
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

    double acc = 0.0;                              // this lane's share of sum(g^2), added in index order
    if (aligned) {
        const int nvec = n >> 2;
        if (n == BMC_ADAM_CHUNK) vec_pass<AMS, NORM, true>(p, g, m, v, x, nvec, tid, k, acc);     // all loads in flight, then the arithmetic
        else vec_pass<AMS, NORM, false>(p, g, m, v, x, nvec, tid, k, acc);
        const int e = 4 * nvec + tid;              // the last partial vector, one element per lane
        if (e < n) {
            const float ge = gld<float>(g + e);
            float pe = gld<float>(p + e), me = gld<float>(m + e), ve = gld<float>(v + e), xe = AMS ? gld<float>(x + e) : 0.f;
            if constexpr (NORM) acc += sq(ge);
            adam_elem<AMS>(pe, ge, me, ve, xe, k);
            gst<float>(p + e, pe); gst<float>(m + e, me); gst<float>(v + e, ve);
            if constexpr (AMS) gst<float>(x + e, xe);
        }
    } else {
        for (int e = tid; e < n; e += AT) {
            const float ge = gld<float>(g + e);
            float pe = gld<float>(p + e), me = gld<float>(m + e), ve = gld<float>(v + e), xe = AMS ? gld<float>(x + e) : 0.f;
            if constexpr (NORM) acc += sq(ge);
            adam_elem<AMS>(pe, ge, me, ve, xe, k);
            gst<float>(p + e, pe); gst<float>(m + e, me); gst<float>(v + e, ve);
            if constexpr (AMS) gst<float>(x + e, xe);
        }
    }
    if constexpr (NORM) {                          // a fixed tree over the workgroup
        __shared__ double red[AT];
        const double total = tree_sum(red, acc, tid);
        if (tid == 0) gst<double>(partial_sq + blockIdx.x, total);
    }
}

// the second launch of the capturable entry point: one lane, a plain vector store
__global__ void adam_advance_kernel(int* __restrict__ step_dev) {
    if (threadIdx.x == 0) gst<int>(step_dev, gld<int>(step_dev) + 1);
}

typedef void (*adam_fn)(const bmc_adam_chunk_t*, const bmc_adam_hyper_t, const int*, double*);
template <bool CAP>
adam_fn adam_pick(bool ams, bool norm) {
    if (ams) return norm ? adam_kernel<true, true, CAP> : adam_kernel<true, false, CAP>;
    return norm ? adam_kernel<false, true, CAP> : adam_kernel<false, false, CAP>;
}

}  // namespace

extern "C" int bmc_adam_step(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, double* partial_sq, bmc_stream_t s) {
    if (adam_check("bmc_adam_step", table, n_chunks, hyper, false)) return -1;
    if (n_chunks == 0) return 0;
    const adam_fn fn = adam_pick<false>(hyper.amsgrad != 0, partial_sq != nullptr);
    hipLaunchKernelGGL(fn, dim3((unsigned)n_chunks), dim3(AT), 0, (hipStream_t)s, table, hyper, (const int*)nullptr, partial_sq);
    BMC_CHECK_LAUNCH("bmc_adam_step");
    return 0;
}

extern "C" int bmc_adam_step_capturable(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, int* step_dev,
                                        double* partial_sq, bmc_stream_t s) {
    if (adam_check("bmc_adam_step_capturable", table, n_chunks, hyper, true)) return -1;
    BMC_CHECK_ARG(step_dev || n_chunks == 0, "bmc_adam_step_capturable: no step counter");
    if (n_chunks == 0) return 0;
    const adam_fn fn = adam_pick<true>(hyper.amsgrad != 0, partial_sq != nullptr);
    hipLaunchKernelGGL(fn, dim3((unsigned)n_chunks), dim3(AT), 0, (hipStream_t)s, table, hyper, (const int*)step_dev, partial_sq);
    BMC_CHECK_LAUNCH("bmc_adam_step_capturable");
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, step_dev);
    BMC_CHECK_LAUNCH("bmc_adam_step_capturable");
    return 0;
}
