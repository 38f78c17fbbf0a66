// Optimizer step (bmcnet-esr_amd/bmc_hip/optim.py::Adam): torch.optim.Adam(amsgrad, weight_decay) for every parameter of a group in
// ONE launch over a device table of chunks, and its clipped form (Adam(max_grad_norm=, nonfinite=)): a norm launch, then a step
// launch that clips by the global gradient norm or skips a non-finite step without a host round trip.  The contract -- the six
// roundings per element, the chunk table, the gradient-norm partials, the coefficient, the capturable variants -- is stated once in
// include/bmc_hip.h "optimizer step" and "optimizer step: clipping".
//
// An HBM-bound element-wise pass: 36 bytes per element (read p, g, m, v, vmax; write p, m, v, vmax), each touched once; the norm
// launch reads g alone (4 bytes per element).  A workgroup of 256 lanes owns one chunk of at most 4096 elements of one tensor: a
// lane issues its (up to) 20 16-byte loads, then computes, then stores.  The table's pointers are made wave-uniform (readfirstlane)
// and every access goes through the address-space(1) accessors of slot_k.h: scalar base + lane offset, global_* instructions, never
// flat_*.  No workgroup waits for another, no atomics, no scratch memory.  The kernels below are shells: the walk over a chunk, the
// element arithmetic, the set-up of the constants, the unclipped body and the clipped head are in adam_k.h, once.  These are the
// EMA = false instantiations; optim_ema.hip holds the EMA = true ones (include/bmc_hip_ema.h).
#include "adam_k.h"

namespace {

// grid: n_chunks workgroups.  AMS: amsgrad; NORM: partial_sq is given; CAP: the step count comes from *step_dev.
template <bool AMS, bool NORM, bool CAP>
__global__ __launch_bounds__(AT) void adam_kernel(const bmc_adam_chunk_t* __restrict__ table, const bmc_adam_hyper_t h,
                                                  const int* __restrict__ step_dev, double* __restrict__ partial_sq) {
    adam_body<AMS, NORM, CAP, false>(table, h, step_dev, partial_sq, NoEma{});
}

// the norm launch of a clipped step: the partials adam_kernel<.., NORM = true, ..> stores, from g alone
__global__ __launch_bounds__(AT) void grad_sq_kernel(const bmc_adam_chunk_t* __restrict__ table, double* __restrict__ partial_sq) {
    __shared__ double red[AT];
    const int tid = threadIdx.x;
    const double total = tree_sum(red, grad_sq_chunk(chunk_view<false>(table + blockIdx.x), tid), tid);
    if (tid == 0) gst<double>(partial_sq + blockIdx.x, total);
}

// The step launch of a clipped step.  grid: n_chunks workgroups.  AMS: amsgrad; CAP: the step count comes from *step_dev.
template <bool AMS, bool CAP>
__global__ __launch_bounds__(AT) void clip_step_kernel(const bmc_adam_chunk_t* __restrict__ table, const bmc_adam_hyper_t h,
                                                       const int* __restrict__ step_dev, const bmc_adam_clip_t clip) {
    __shared__ double red[AT];
    const int tid = threadIdx.x;
    const Chunk ck = chunk_view<AMS>(table + blockIdx.x);
    BMC_CLIP_STEP_HEAD(clip, red, tid);            // nothing of p, m, v, vmax is stored

    // The partials are reduced BEFORE the chunk's loads are issued: step_chunk comes last.  Issuing a full chunk's 20 loads first, so
    // that the reduction runs under their latency, holds 80 registers across the reduction and its barriers.  On the layout this
    // kernel had when it was a translation unit of its own (194 VGPRs, occupancy 2) that order was measured and was slower: 248
    // VGPRs, one wave per SIMD fewer, 24.6 against 17.6 us for the BMCNet(4,128,5) set on an MI355X.  On the shared walk the kernel
    // stands at 126-128 VGPRs with amsgrad (110-112 without), occupancy 4, and takes 16.0 us for that set; the other order has not
    // been measured on it.
    const AdamK k = adam_setup<CAP, false>(h, step_dev, tid, NoEma{});
    step_chunk<AMS, false>(ck, tid, k, GradClipped{c});
}

// the last launch of the capturable entry points: one lane, a plain vector store (also after a skipped step)
__global__ void adam_advance_kernel(int* __restrict__ step_dev) {
    if (threadIdx.x == 0) gst<int>(step_dev, gld<int>(step_dev) + 1);
}

typedef void (*adam_fn)(const bmc_adam_chunk_t*, const bmc_adam_hyper_t, const int*, double*);
template <bool CAP>
adam_fn adam_pick(bool ams, bool norm) {
    if (ams) return norm ? adam_kernel<true, true, CAP> : adam_kernel<true, false, CAP>;
    return norm ? adam_kernel<false, true, CAP> : adam_kernel<false, false, CAP>;
}

bool finite_f(float v) { return isfinite(v); }

}  // namespace

// ---- host: the argument checks the entry points make before they launch (declared in adam_k.h: optim_ema.hip calls them too)
namespace bmc_adam_host {

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

int clip_check(const char* name, int n_chunks, const bmc_adam_clip_t& clip) {
    BMC_CHECK_ARG(clip.partial_sq || n_chunks == 0, "%s: no partial_sq (the norm launches of the step write it)", name);
    BMC_CHECK_ARG(clip.n_partials >= n_chunks, "%s: n_partials = %d is less than n_chunks = %d", name, clip.n_partials, n_chunks);
    BMC_CHECK_ARG(clip.max_norm > 0.f, "%s: max_norm = %g is not a positive number (+INF: never clip)", name, clip.max_norm);
    BMC_CHECK_ARG(clip.skip_nonfinite == 0 || clip.skip_nonfinite == 1, "%s: skip_nonfinite = %d is neither 0 nor 1", name,
                  clip.skip_nonfinite);
    return 0;
}

// the second launch of every capturable entry point
int advance(const char* name, int* step_dev, bmc_stream_t s) {
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, step_dev);
    BMC_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace bmc_adam_host

using namespace bmc_adam_host;

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
    return advance("bmc_adam_step_capturable", step_dev, s);
}

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
    return advance("bmc_adam_step_clipped_capturable", step_dev, s);
}
