/* bmc_hip_quality.h -- companion of bmc_hip.h: PSNR and SSIM of a window of multi-stream inference, per slot, on the GPU.
 *
 * bmc_slot_metrics (bmc_hip.h) gives the MSE column of a super-resolution table; the entry point below gives the other two, the
 * reference's psnr_loss / ssim_loss (loss/restore.py:44-93, wrappers around scikit-image run per channel on the CPU).  It is
 * exported by the same library (csrc/slot_quality.hip) and described, as text made by the compiler from these declarations, by
 * bmc_quality_abi() -- the records of bmc_abi() (csrc/abi.hip) -- from which bmc_hip/quality_lib.py builds its binding.
 * bmc_hip.h itself is unchanged by it.
 *
 * DEFINITIONS (the contract).  Both metrics are taken per channel c of a two-channel count image: an image a against the
 * window's ground truth g, both float32 [2][gh][gw].  All arithmetic is float64 on the float32 inputs, as scikit-image computes
 * after its astype(float64); the result of a window is the mean of the two channels (restore.py:56-61, :80-87).
 *   Data range  R_c = max(g[c]) - min(g), the minimum over BOTH channels (restore.py:85: tgt[idx].max() - tgt.min()), or a
 *               positive constant the caller gives.
 *   PSNR        mse_c = sum ((double) a - (double) g)^2 / (gh * gw);  psnr_c = 10 log10(R_c^2 / mse_c), finished on the host
 *               (scikit-image's peak_signal_noise_ratio).  IEEE results stand: +inf for an exact channel, -inf for R_c = 0 with
 *               an error, nan for 0 / 0.
 *   SSIM        scikit-image's structural_similarity with its defaults: a uniform BMC_QUALITY_WIN x BMC_QUALITY_WIN window,
 *               K1 = 0.01, K2 = 0.03, C1 = (K1 R_c)^2, C2 = (K2 R_c)^2, sample covariance.  With the 49-term sums s_x, s_y,
 *               s_xx, s_yy, s_xy of a window position (x = a, y = g):
 *                   ux = s_x / 49, uy = s_y / 49, vx = (s_xx - s_x^2 / 49) / 48, vy, vxy likewise,
 *                   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),
 *               every operation rounded on its own.  ssim_c = the mean of S over the (gh - 6) x (gw - 6) window positions that
 *               lie wholly inside the image (scikit-image crops (win - 1) / 2 at every border, so its boundary mode never
 *               enters).  R_c == 0: ssim_c = NaN (scikit-image has no defined value there).  gh, gw >= BMC_QUALITY_WIN.
 *
 * The raw record of a window is double [2 images][2 channels][BMC_QUALITY_WORDS] = {sse, gt_max, gt_min, ssim_sum}: sse = the
 * sum of mse_c, gt_max = max(g[c]), gt_min = min(g) (both channels), ssim_sum = the sum of S over the window positions (NaN for
 * R_c == 0).  128 bytes per window; the host finishes them (bmc_hip.slots.quality_values). */
#ifndef BMC_HIP_QUALITY_H
#define BMC_HIP_QUALITY_H

#include "bmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BMC_QUALITY_WIN 7
#define BMC_QUALITY_WORDS 4         /* doubles per (image, channel) of a raw record */
#define BMC_QUALITY_TILE_H 32       /* window positions a workgroup of the ssim launch owns: rows ... */
#define BMC_QUALITY_TILE_W 64       /* ... and columns */
#define BMC_QUALITY_STATS_WORDS 8   /* doubles per (slot, part) of the stats scratch */

/* The quality entry of a slot: a DEVICE table of S entries parallel to the slot table. */
typedef struct bmc_slot_quality {
    double* dst;            /* NULL (skip the slot), or where the window's raw record [2][2][BMC_QUALITY_WORDS] goes */
} bmc_slot_quality_t;

/* Every active slot (bmc_slot_t: BMC_SLOT_ACTIVE, frames set) with a quality entry and a ground truth: the raw records of the
 * images esr[s] and bicubic[s] ([S][2][gh][gw] float32 each, already at the ground truth's size) against the slot entry's gt.
 * bicubic NULL: image 0 only, words of image 1 are not written.  data_range > 0: R_c is that constant; data_range == 0: R_c from
 * the ground truth (gt_max / gt_min are written either way).  Three launches for all slots:
 *   stats   grid (nparts, S), 1 <= nparts <= BMC_SLOT_MAX_PARTS: part p's fixed element set (element i of [2][gh][gw] in part
 *           (i / 1024) % nparts, as bmc_slot_metrics) -> per channel the sse of each image in double, max(g[c]), min(g), reduced
 *           in a fixed tree -> stats [S][nparts][BMC_QUALITY_STATS_WORDS] = {sse[image][channel] x 4, max[channel] x 2, min, 0};
 *   ssim    grid (tiles, images x 2, S): a workgroup owns BMC_QUALITY_TILE_H x BMC_QUALITY_TILE_W window positions of one
 *           channel of one image; it folds the slot's max / min parts to R_c, stages its tile with a 6-pixel apron in LDS,
 *           forms the five 49-term sums separably in double (row sums left to right, then the seven rows top to bottom),
 *           evaluates S, reduces the tile in a fixed tree -> tiles [S][4][ntiles], ntiles = ceil((gh - 6) / TILE_H) *
 *           ceil((gw - 6) / TILE_W); positions outside a ragged tile add exact zeros;
 *   finish  one workgroup per (slot, image, channel): the stats parts and the tile partials added in index order -> dst.
 * No atomics, no workgroup waits for another, nothing a slot computes depends on another slot, no host read: bit-reproducible.
 * Refused before any launch: null table / quality / esr / stats / tiles, S outside 1 .. BMC_MAX_SLOTS, gh or gw below
 * BMC_QUALITY_WIN, 2 * gh * gw >= 2^30, nparts out of range, a data_range that is negative or not finite, stats / tiles not
 * 8-byte aligned. */
int bmc_slot_quality(const bmc_slot_t* table, const bmc_slot_quality_t* quality, int S, const float* esr, const float* bicubic,
                     int gh, int gw, int nparts, double data_range, double* stats, double* tiles, bmc_stream_t s);

/* The ABI text of this header: fn, struct, field and const records as bmc_abi() writes them. */
const char* bmc_quality_abi(void);

#ifdef __cplusplus
}
#endif

#endif /* BMC_HIP_QUALITY_H */
