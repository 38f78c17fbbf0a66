/* bmc_hip_ssim.h -- companion of bmc_hip.h: the structural training loss 1 - mean SSIM and its gradient, on the GPU.
 *
 * bmc_hip_quality.h scores a window of inference with SSIM; the two entry points below are the differentiable form of the same
 * quantity for training, with a constant data range.  They are exported by the same library (csrc/ssim_loss.hip) and described,
 * as text made by the compiler from these declarations, by bmc_ssim_abi() -- the records of bmc_abi() (csrc/abi.hip) -- from
 * which bmc_hip/ssim_lib.py builds its binding.  bmc_hip.h itself is unchanged by them.
 *
 * DEFINITION (the contract).  x (the prediction) and y (the ground truth) are float32 [B][C][h][w], h, w >= BMC_SSIM_WIN.  All
 * arithmetic is float64 on the float32 inputs, every operation rounded on its own.  The window is uniform BMC_SSIM_WIN x
 * BMC_SSIM_WIN: n = 49, cn = n / (n - 1) = 49 / 48.  K1 = 0.01, K2 = 0.03, C1 = (K1 R)^2, C2 = (K2 R)^2 with R = data_range > 0 a
 * finite constant.  The window positions are the (h - 6)(w - 6) per plane that lie wholly inside the image.  With the 49-term
 * sums s_x, s_y, s_xx, s_yy, s_xy of a position (SUMMATION ORDER: the seven terms of a window row left to right, then the seven
 * row sums top to bottom):
 *     ux = s_x / n, uy = s_y / n, vx = (s_xx - s_x s_x / n) / (n - 1), vy, vxy likewise,
 *     A1 = 2 ux uy + C1,  A2 = 2 vxy + C2,  B1 = ux ux + uy uy + C1,  B2 = vx + vy + C2,  D = B1 B2,
 *     S  = (A1 A2) / D,
 *     loss = 1 - (sum of S over all count = B C (h - 6)(w - 6) positions) / count, rounded to float32 once.
 * GRADIENT.  Every position carries three coefficients, with k = (2 cn) / n,
 *     gamma = -(k S) / B2,   beta = (k (A1 / B1)) / B2,
 *     alpha = (((2 uy) / B1) (A2 / B2) - (2 ux S) / B1) / n - beta uy - gamma ux
 * (gamma = -2 cn S / (n B2), beta = 2 cn A1 / (n B1 B2), alpha = (2 uy A2 / (B1 B2) - 2 ux S / B1) / n - beta uy - gamma ux,
 * evaluated in the order written so that x == y gives A1 / B1 = A2 / B2 = S = 1, beta = -gamma and alpha = 0 EXACTLY),
 * and with sa, sb, sg the sums of alpha, beta, gamma over the positions whose window holds pixel i (the position rows i_y - 6 ..
 * i_y, the columns i_x - 6 .. i_x, a position outside the image adding an exact zero; ORDER: the seven columns of a position row
 * left to right, then the seven row sums top to bottom)
 *     dloss/dx[i] = -((sa + y[i] sb) + x[i] sg) / count,
 * multiplied by the upstream scalar gradient in float64 and rounded to float32 once.  IEEE values stand; two all-zero windows have
 * S = 1, alpha = 0 and a zero gradient; x == y bit for bit gives loss 0 and a gradient of exact zeros. */
#ifndef BMC_HIP_SSIM_H
#define BMC_HIP_SSIM_H

#include "bmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BMC_SSIM_WIN 7
#define BMC_SSIM_TILE_H 32          /* forward: window positions a workgroup owns, rows ... */
#define BMC_SSIM_TILE_W 64          /* ... and columns */
#define BMC_SSIM_BWD_TILE_H 16      /* backward: pixels a workgroup owns, rows ... */
#define BMC_SSIM_BWD_TILE_W 32      /* ... and columns */

/* loss[0] (DEVICE float32) = 1 - mean SSIM of x [B][C][h][w] (contiguous) against y (contiguous planes and channels, batch
 * stride y_batch_stride >= C h w elements).  Two launches:
 *   tiles   a workgroup owns BMC_SSIM_TILE_H x BMC_SSIM_TILE_W window positions of one plane: the tile and its 6-pixel apron staged
 *           in LDS as float32, the five sums formed separably in double in the order above, S per position; a lane adds the S
 *           of its column of the wave's strip of TILE_H / 4 rows top to bottom, the 64 lanes fold in a tree (lane l += lane l + o,
 *           o = 32, 16, ..., 1), the four waves add as ((w0 + w1) + w2) + w3; positions outside a ragged tile add exact zeros
 *           -> tiles [B C][ntiles], ntiles = ceil((h - 6) / TILE_H) * ceil((w - 6) / TILE_W), tile index row-major;
 *   finish  one workgroup adds the B C ntiles partials in index order and writes 1 - sum / count.
 * tiles: caller-provided scratch of B C ntiles doubles.
 * Refused before any launch (-1): null x / y / tiles / loss, B or C below 1, h or w below BMC_SSIM_WIN, B C h w >= 2^30, a
 * data_range that is not positive and finite, tiles not 8-byte aligned, y_batch_stride below C h w, B C ntiles >= 2^23. */
int bmc_ssim_loss_fwd(const float* x, const float* y, long long y_batch_stride, int B, int C, int h, int w, double data_range,
                      double* tiles, float* loss, bmc_stream_t s);

/* dx [B][C][h][w] (contiguous float32) = gloss[0] * dloss/dx, gloss a DEVICE float32 scalar.  ONE launch; nothing of the forward
 * is read but x and y: a workgroup owns BMC_SSIM_BWD_TILE_H x BMC_SSIM_BWD_TILE_W PIXELS of one plane, stages x and y with 6 pixels
 * of apron on each side (zeros outside the image), recomputes alpha, beta, gamma in double in LDS for the (TILE_H + 6) x
 * (TILE_W + 6) positions that touch its pixels, and gathers per pixel in the order above.  Every element of dx is written once.
 * Refused before any launch (-1): null x / y / gloss / dx, and the forward's conditions on B, C, h, w, data_range and
 * y_batch_stride; the number of workgroups B C ceil(h / TILE_H) ceil(w / TILE_W) must be below 2^23. */
int bmc_ssim_loss_bwd(const float* x, const float* y, long long y_batch_stride, const float* gloss, int B, int C, int h, int w,
                      double data_range, float* dx, bmc_stream_t s);

/* The ABI text of this header: fn and const records as bmc_abi() writes them. */
const char* bmc_ssim_abi(void);

#ifdef __cplusplus
}
#endif

#endif /* BMC_HIP_SSIM_H */
