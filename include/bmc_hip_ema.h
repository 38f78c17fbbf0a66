/* bmc_hip_ema.h -- companion of bmc_hip.h: an exponential moving average (EMA) of the weights inside the optimizer step, and the
 * in-place exchange of weights and averages for validation (bmcnet-esr_amd/bmc_hip/optim.py::Adam(ema_decay=, ema_warmup=)).
 *
 * The entry points below are exported by the same library (csrc/optim_ema.hip; the walk over a chunk and the element functions are
 * those of csrc/adam_k.h, shared with csrc/optim.hip) and described, as text made by the compiler from these declarations, by
 * bmc_ema_abi() -- the records of bmc_abi() (csrc/abi.hip) -- from which bmc_hip/ema_lib.py builds its binding.  bmc_hip.h itself,
 * bmc_adam_chunk_t and bmc_adam_hyper_t among it, is unchanged.
 *
 * optimizer step with EMA (the contract).  Each of the four step entry points of bmc_hip.h "optimizer step" and "optimizer step:
 * clipping" has a twin here that takes one more argument, a bmc_adam_ema_t.  A twin does everything its original does, with the
 * same roundings: p, m, v and vmax come out bit for bit as from the original.  In the SAME launch, after the six lines have produced
 * the new p of an element, three more lines run on the element's average e, in float32, every line ONE correctly rounded operation
 * (no fused multiply-add):
 *     d = p - e                        p: the new value
 *     s = w * d
 *     e = e + s
 * NaN and Inf propagate as the formulas say; subnormals are kept.  44 bytes per element instead of 36 (amsgrad): e is read with the
 * other streams and written with the other stores, through the same global accessors; no atomics, no scratch, no added launch.
 * The weight.  decay is a float64 in [0, 1).  For the step whose 1-based count is t -- the t of the bias corrections --
 *     decay_t = warmup ? min(decay, t / (t + 9)) : decay          float64; (1 + n) / (10 + n) with n = t - 1 earlier updates
 *     w       = (float) (1.0 - decay_t)                           float64 subtraction, rounded to float32 ONCE
 * The plain twins take w as the host computed it (the field `w`; decay and warmup are only checked).  The capturable twins ignore
 * the field: the lane of each workgroup that computes the two bias corrections from *step_dev computes w from t = *step_dev + 1
 * with the same float64 operations (a division, a minimum and a subtraction, all exactly rounded), so both forms give the same bits.
 * Skipped steps.  In the clipped twins the uniform skip of a step whose gradients are not finite (skip_nonfinite == 1) comes before
 * everything else: a skipped step stores nothing to e, exactly as to p, m, v and vmax.  A skipped step still counts as a step for
 * t, in the decay schedule as in the bias corrections: the average that follows it uses the decay of one step later.
 * e, the EMA pointer array, is a DEVICE array parallel to the chunk table: entry i belongs to chunk i and already points at the
 * chunk's first element (the tensor's average plus the chunk's element offset).  `aligned` != 0 in chunk i now ALSO promises that
 * e[i] is 16-byte aligned.  The capturable twins are followed by the same advance launch as their originals.
 * Checked: everything the original checks; e non-NULL where n_chunks > 0; decay finite and in [0, 1); warmup 0 or 1; for the plain
 * twins w finite.  Trusted: the pointers of the table and of e.
 *
 * bmc_ema_swap exchanges p and e of every chunk in place, bit for bit: 16 bytes per element, whole 16-byte vectors where the
 * chunk is `aligned` and single elements otherwise, over the same walk.  Applied twice it is the identity.  It reads only the p and
 * n fields (and `aligned`) of a chunk and the EMA pointer. */
#ifndef BMC_HIP_EMA_H
#define BMC_HIP_EMA_H

#include "bmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bmc_adam_ema {
    float* const* e;        /* DEVICE array [n_chunks]: the average of chunk i, at the chunk's first element */
    double decay;           /* [0, 1) */
    float w;                /* (float)(1 - decay_t) of this step; ignored by the capturable entry points */
    int warmup;             /* 0 or 1: decay_t = min(decay, t / (t + 9)) */
} bmc_adam_ema_t;

int bmc_adam_ema_step(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, bmc_adam_ema_t ema, double* partial_sq,
                      bmc_stream_t s);
int bmc_adam_ema_step_capturable(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, bmc_adam_ema_t ema,
                                 int* step_dev, double* partial_sq, bmc_stream_t s);
int bmc_adam_ema_step_clipped(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, bmc_adam_ema_t ema,
                              bmc_adam_clip_t clip, bmc_stream_t s);
int bmc_adam_ema_step_clipped_capturable(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, bmc_adam_ema_t ema,
                                         int* step_dev, bmc_adam_clip_t clip, bmc_stream_t s);

/* Checked: n_chunks >= 0 (0: nothing is launched), a table and an EMA array when n_chunks > 0.  Trusted: the pointers. */
int bmc_ema_swap(const bmc_adam_chunk_t* table, float* const* e, int n_chunks, bmc_stream_t s);

/* The ABI text of this header: fn, struct and field records as bmc_abi() writes them. */
const char* bmc_ema_abi(void);

#ifdef __cplusplus
}
#endif

#endif /* BMC_HIP_EMA_H */
