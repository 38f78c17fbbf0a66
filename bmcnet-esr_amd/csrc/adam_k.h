// The element arithmetic of the optimizer step, shared by optim.hip (bmc_adam_step) and optim_clip.hip (the clipped step): both
// translation units round alike because they compile THIS adam_elem.  Internal; the contract is include/bmc_hip.h "optimizer step".
#pragma once
#include <math.h>
#include "bmc_common.h"
#include "slot_k.h"

namespace {

constexpr int AT = 256;                            // lanes per workgroup
constexpr int VPL = BMC_ADAM_CHUNK / 4 / AT;       // 16-byte vectors per lane of a full chunk
static_assert(VPL * 4 * AT == BMC_ADAM_CHUNK, "a full chunk is a whole number of rounds of the workgroup");

struct AdamK {
    float omb1, beta2, omb2, eps, wd, step_size, bc2s;
};

// One element.  Both load paths call this, so they round alike.  sqrt and the divisions are the compiler's own operators: in a HIP
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

// ---- host: the argument checks every entry point of the family makes before it launches
bool finite_f(float v) { return isfinite(v); }

int adam_check(const char* name, const bmc_adam_chunk_t* table, int n_chunks, const bmc_adam_hyper_t& h, bool cap) {
    BMC_CHECK_ARG(n_chunks >= 0, "%s: n_chunks = %d is negative", name, n_chunks);
    BMC_CHECK_ARG(table || n_chunks == 0, "%s: no chunk table for %d chunks", name, n_chunks);
    BMC_CHECK_ARG(finite_f(h.beta1) && finite_f(h.one_minus_beta1) && finite_f(h.beta2) && finite_f(h.one_minus_beta2) &&
                      finite_f(h.eps) && finite_f(h.weight_decay),
                  "%s: a hyper-parameter is not finite (beta1 %g, 1 - beta1 %g, beta2 %g, 1 - beta2 %g, eps %g, weight_decay %g)", name,
                  h.beta1, h.one_minus_beta1, h.beta2, h.one_minus_beta2, h.eps, h.weight_decay);
    if (cap)
        BMC_CHECK_ARG(isfinite(h.lr) && isfinite(h.beta1_f64) && isfinite(h.beta2_f64),
                      "%s: a hyper-parameter is not finite (lr %g, beta1 %g, beta2 %g)", name, h.lr, h.beta1_f64, h.beta2_f64);
    else
        BMC_CHECK_ARG(finite_f(h.step_size) && finite_f(h.bias_correction2_sqrt),
                      "%s: a hyper-parameter is not finite (step_size %g, bias_correction2_sqrt %g)", name, h.step_size,
                      h.bias_correction2_sqrt);
    return 0;
}

}  // namespace
