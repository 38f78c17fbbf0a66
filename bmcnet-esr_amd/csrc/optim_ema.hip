// Optimizer step with an exponential moving average of the weights (bmcnet-esr_amd/bmc_hip/optim.py::Adam(ema_decay=, ema_warmup=)):
// the EMA = true instantiations of the step kernels of optim.hip, and the in-place exchange of weights and averages.  The contract
// -- the three roundings per element on top of the step's, the decay schedule, the skip rule, the EMA pointer array -- is stated once
// in include/bmc_hip_ema.h.
//
// The same HBM-bound pass as optim.hip with one more stream: 44 bytes per element instead of 36 (read and write e).  A lane of a full
// chunk issues 24 16-byte loads instead of 20 before it computes.  The kernels are shells over the bodies of adam_k.h: the walk, the
// element arithmetic of p, m, v and vmax, the reduction of a clipped step and its uniform skip are the ones optim.hip compiles, so
// p, m, v and vmax come out as from the kernels there, bit for bit.  No workgroup waits for another, no atomics, no scratch memory.
#include "adam_k.h"

namespace {

template <bool AMS, bool NORM, bool CAP>
__global__ __launch_bounds__(AT) void adam_ema_kernel(const bmc_adam_chunk_t* __restrict__ table, const bmc_adam_hyper_t h,
                                                      const bmc_adam_ema_t ema, const int* __restrict__ step_dev,
                                                      double* __restrict__ partial_sq) {
    adam_body<AMS, NORM, CAP, true>(table, h, step_dev, partial_sq, ema);
}

template <bool AMS, bool CAP>
__global__ __launch_bounds__(AT) void clip_step_ema_kernel(const bmc_adam_chunk_t* __restrict__ table, const bmc_adam_hyper_t h,
                                                           const bmc_adam_ema_t ema, const int* __restrict__ step_dev,
                                                           const bmc_adam_clip_t clip) {
    __shared__ double red[AT];
    const int tid = threadIdx.x;
    Chunk ck = chunk_view<AMS>(table + blockIdx.x);
    ck.e = uniform_ptr<float>(ema.e + blockIdx.x);
    BMC_CLIP_STEP_HEAD(clip, red, tid);            // nothing of p, m, v, vmax or e is stored
    const AdamK k = adam_setup<CAP, true>(h, step_dev, tid, ema);      // after the reduction, as in clip_step_kernel
    step_chunk<AMS, true>(ck, tid, k, GradClipped{c});
}

// grid: n_chunks workgroups.  p and e of every chunk exchanged; of the table's entry only p, n and aligned are read.
__global__ __launch_bounds__(AT) void ema_swap_kernel(const bmc_adam_chunk_t* __restrict__ table, float* const* __restrict__ ema) {
    const bmc_adam_chunk_t* ent = table + blockIdx.x;
    Chunk ck;
    ck.p = uniform_ptr<float>(&ent->p);
    ck.e = uniform_ptr<float>(ema + blockIdx.x);
    ck.g = nullptr; ck.m = ck.v = ck.x = nullptr;
    const int n = __builtin_amdgcn_readfirstlane(gld<int>(&ent->n));
    ck.n = n < BMC_ADAM_CHUNK ? n : BMC_ADAM_CHUNK;
    ck.aligned = __builtin_amdgcn_readfirstlane(gld<int>(&ent->aligned)) != 0;
    swap_chunk(ck, threadIdx.x);
}

typedef void (*adam_ema_fn)(const bmc_adam_chunk_t*, const bmc_adam_hyper_t, const bmc_adam_ema_t, const int*, double*);
template <bool CAP>
adam_ema_fn adam_ema_pick(bool ams, bool norm) {
    if (ams) return norm ? adam_ema_kernel<true, true, CAP> : adam_ema_kernel<true, false, CAP>;
    return norm ? adam_ema_kernel<false, true, CAP> : adam_ema_kernel<false, false, CAP>;
}

int ema_check(const char* name, int n_chunks, const bmc_adam_ema_t& ema, bool cap) {
    BMC_CHECK_ARG(ema.e || n_chunks <= 0, "%s: no EMA pointer array for %d chunks", name, n_chunks);
    BMC_CHECK_ARG(isfinite(ema.decay) && ema.decay >= 0.0 && ema.decay < 1.0, "%s: the EMA decay = %g is not a finite number in [0, 1)",
                  name, ema.decay);
    BMC_CHECK_ARG(ema.warmup == 0 || ema.warmup == 1, "%s: the EMA warmup flag = %d is neither 0 nor 1", name, ema.warmup);
    if (!cap) BMC_CHECK_ARG(isfinite(ema.w), "%s: the EMA weight w = %g is not finite", name, ema.w);
    return 0;
}

}  // namespace

using namespace bmc_adam_host;

extern "C" int bmc_adam_ema_step(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, bmc_adam_ema_t ema,
                                 double* partial_sq, bmc_stream_t s) {
    if (adam_check("bmc_adam_ema_step", table, n_chunks, hyper, false)) return -1;
    if (ema_check("bmc_adam_ema_step", n_chunks, ema, false)) return -1;
    if (n_chunks == 0) return 0;
    const adam_ema_fn fn = adam_ema_pick<false>(hyper.amsgrad != 0, partial_sq != nullptr);
    hipLaunchKernelGGL(fn, dim3((unsigned)n_chunks), dim3(AT), 0, (hipStream_t)s, table, hyper, ema, (const int*)nullptr, partial_sq);
    BMC_CHECK_LAUNCH("bmc_adam_ema_step");
    return 0;
}

extern "C" int bmc_adam_ema_step_capturable(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, bmc_adam_ema_t ema,
                                            int* step_dev, double* partial_sq, bmc_stream_t s) {
    if (adam_check("bmc_adam_ema_step_capturable", table, n_chunks, hyper, true)) return -1;
    if (ema_check("bmc_adam_ema_step_capturable", n_chunks, ema, true)) return -1;
    BMC_CHECK_ARG(step_dev || n_chunks == 0, "bmc_adam_ema_step_capturable: no step counter");
    if (n_chunks == 0) return 0;
    const adam_ema_fn fn = adam_ema_pick<true>(hyper.amsgrad != 0, partial_sq != nullptr);
    hipLaunchKernelGGL(fn, dim3((unsigned)n_chunks), dim3(AT), 0, (hipStream_t)s, table, hyper, ema, (const int*)step_dev, partial_sq);
    BMC_CHECK_LAUNCH("bmc_adam_ema_step_capturable");
    return advance("bmc_adam_ema_step_capturable", step_dev, s);
}

extern "C" int bmc_adam_ema_step_clipped(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, bmc_adam_ema_t ema,
                                         bmc_adam_clip_t clip, bmc_stream_t s) {
    if (adam_check("bmc_adam_ema_step_clipped", table, n_chunks, hyper, false)) return -1;
    if (clip_check("bmc_adam_ema_step_clipped", n_chunks, clip)) return -1;
    if (ema_check("bmc_adam_ema_step_clipped", n_chunks, ema, false)) return -1;
    if (n_chunks == 0) return 0;
    const auto fn = hyper.amsgrad != 0 ? clip_step_ema_kernel<true, false> : clip_step_ema_kernel<false, false>;
    hipLaunchKernelGGL(fn, dim3((unsigned)n_chunks), dim3(AT), 0, (hipStream_t)s, table, hyper, ema, (const int*)nullptr, clip);
    BMC_CHECK_LAUNCH("bmc_adam_ema_step_clipped");
    return 0;
}

extern "C" int bmc_adam_ema_step_clipped_capturable(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper,
                                                    bmc_adam_ema_t ema, int* step_dev, bmc_adam_clip_t clip, bmc_stream_t s) {
    if (adam_check("bmc_adam_ema_step_clipped_capturable", table, n_chunks, hyper, true)) return -1;
    if (clip_check("bmc_adam_ema_step_clipped_capturable", n_chunks, clip)) return -1;
    if (ema_check("bmc_adam_ema_step_clipped_capturable", n_chunks, ema, true)) return -1;
    BMC_CHECK_ARG(step_dev || n_chunks == 0, "bmc_adam_ema_step_clipped_capturable: no step counter");
    if (n_chunks == 0) return 0;
    const auto fn = hyper.amsgrad != 0 ? clip_step_ema_kernel<true, true> : clip_step_ema_kernel<false, true>;
    hipLaunchKernelGGL(fn, dim3((unsigned)n_chunks), dim3(AT), 0, (hipStream_t)s, table, hyper, ema, (const int*)step_dev, clip);
    BMC_CHECK_LAUNCH("bmc_adam_ema_step_clipped_capturable");
    return advance("bmc_adam_ema_step_clipped_capturable", step_dev, s);
}

extern "C" int bmc_ema_swap(const bmc_adam_chunk_t* table, float* const* e, int n_chunks, bmc_stream_t s) {
    BMC_CHECK_ARG(n_chunks >= 0, "bmc_ema_swap: n_chunks = %d is negative", n_chunks);
    BMC_CHECK_ARG(table || n_chunks == 0, "bmc_ema_swap: no chunk table for %d chunks", n_chunks);
    BMC_CHECK_ARG(e || n_chunks == 0, "bmc_ema_swap: no EMA pointer array for %d chunks", n_chunks);
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(ema_swap_kernel, dim3((unsigned)n_chunks), dim3(AT), 0, (hipStream_t)s, table, e);
    BMC_CHECK_LAUNCH("bmc_ema_swap");
    return 0;
}
