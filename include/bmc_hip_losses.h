/* bmc_hip_losses.h -- companion of bmc_hip.h: the loss head of a training window with a robust loss.
 *
 * bmc_hip.h's head entry points (bmc_head_mse_*, bmc_head_resize_mse_*) compute nn.MSELoss, the reference's only loss; the two
 * below are the same head with another pointwise function.  They are exported by the same library (csrc/head_resize.hip) and
 * described, as text made by the compiler from these declarations, by bmc_losses_abi() -- the records of bmc_abi()
 * (csrc/abi.hip) -- from which bmc_hip/loss_lib.py builds its binding.  bmc_hip.h itself is unchanged by them. */
#ifndef BMC_HIP_LOSSES_H
#define BMC_HIP_LOSSES_H

#include "bmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Head + a robust loss of one window, for a ground truth gt [B][C][gh][gw] (contiguous planes, batch stride gt_batch_stride) of
 * EITHER size: the arguments of bmc_head_resize_mse_fwd plus the pointwise function rho (`kind`) and its parameter.
 *   pred [B,C,rH,rW]   = pixel_shuffle(xo, r) + bilinear(base): bit for bit what bmc_shuffle_to_hr writes for the same operands,
 *                        whatever the loss (it recurs into the next window).
 *   d                  = pred - gt where (gh, gw) == (rH, rW): no resampling (train.py:227-231 skips the resize);
 *                      = bicubic(pred -> gh x gw) - gt otherwise, taps and summation order of bmc_bicubic_resize_fwd.
 *   loss[0]            = sum rho(d) / (B*C*gh*gw) from per-block partial sums (partials: >= 2048 floats of workspace) added in
 *                        index order: deterministic, no atomics.
 *   kind, param          rho(d)                                                 rho'(d)
 *   BMC_LOSS_L1          |d|                                                    sign(d), sign(0) = 0 (ATen's convention)
 *   BMC_LOSS_HUBER       0.5 d^2 if |d| < delta, else delta (|d| - 0.5 delta)   d if |d| < delta, else delta sign(d)
 *                        (param = delta > 0; F.huber_loss)
 *   BMC_LOSS_CHARBONNIER sqrt(d^2 + eps^2)                                      d / sqrt(d^2 + eps^2)      (param = eps > 0)
 *   (param is not read for BMC_LOSS_L1.)
 * Saved for the backward: dsave [B,C,gh,gw] = d itself, written only where the sizes differ -- the backward applies rho' while it
 * gathers, so one saved tensor serves every kind and rho' is never rounded into memory.  Where the sizes agree dsave is not
 * written (pass NULL): the backward reads pred and gt, as bmc_head_mse_bwd does.  dsave NULL = forward only at either size:
 * nothing of the ground truth's size is stored.
 * Refused before any launch: null xo / base / gt / pred / partials / loss, a non-positive size, an unknown kind, a param that is
 * not a finite positive number for BMC_LOSS_HUBER / BMC_LOSS_CHARBONNIER, rH or rW above 2^31 - 1.  Two launches. */
#define BMC_LOSS_L1 1
#define BMC_LOSS_HUBER 2
#define BMC_LOSS_CHARBONNIER 3
int bmc_head_loss_fwd(const float* xo, int B, int C, int H, int W, int r, const float* base, long long sb, long long sc,
                      long long sy, long long sx, const float* gt, long long gt_batch_stride, int gh, int gw, float* pred,
                      float* dsave, float* partials, float* loss, int kind, float param, bmc_stream_t s);
/* Its backward, one launch: dlr [B,H,W,C*r*r] = pixel_unshuffle(dpred + (gloss[0] / (B*C*gh*gw)) R^T rho'(d)); R^T = the
 * transposed resize as a gather in bmc_bicubic_resize_bwd's order where the sizes differ (d read from dsave), the identity where
 * they agree (d = pred - gt from pred [B,C,rH,rW] and gt with its batch stride; dsave is not read).  dpred NULL = no gradient
 * from the next window; gloss (DEVICE scalar) NULL = no gradient from the loss: a pure permutation of dpred, none of dsave, pred,
 * gt is read.  At least one of the two; with gloss, dsave (sizes differ) or pred and gt (sizes agree) are required.  kind and
 * param are checked as in the forward, whether or not gloss is given. */
int bmc_head_loss_bwd(const float* dpred, const float* dsave, const float* pred, const float* gt, long long gt_batch_stride,
                      const float* gloss, int B, int C, int H, int W, int r, int gh, int gw, int kind, float param, float* dlr,
                      bmc_stream_t s);

/* The ABI text of this header: fn and const records as bmc_abi() writes them. */
const char* bmc_losses_abi(void);

#ifdef __cplusplus
}
#endif

#endif /* BMC_HIP_LOSSES_H */
