// PSNR and SSIM of the slots' windows (MultiStreamSR(quality=...)): the contract is in include/bmc_hip_quality.h.
// bmc_slot_quality gives, per slot with a quality entry, the raw record double [2 images][2 channels][4] = {sse, gt_max, gt_min,
// ssim_sum} of the images esr[s] and bicubic[s] against the slot's ground truth -- what scikit-image's peak_signal_noise_ratio
// and structural_similarity (7x7 uniform window, sample covariance) need of a window, in float64 on the float32 inputs.
//
// THREE launches for all slots; no memset, no atomics, no workgroup waits for another:
//   stats   (nparts, S)            part p of slot s: per channel the squared error of each image, the ground truth's maximum and
//                                  its minimum over its fixed element set -> stats[s][p][8];
//   ssim    (tiles, images*2, S)   a workgroup owns TH x TW window positions of one channel of one image: R_c from the slot's
//                                  parts, then the tile body of ssim_k.h (shared with ssim_loss.hip): the tile and its 6-pixel
//                                  apron staged in LDS as float32, the five 49-term sums formed separably in double, S per
//                                  position and a fixed tree over the tile -> tiles[s][image*2+channel][tile];
//   finish  (images*2, S)          the parts and the tile partials added in index order -> the slot's dst.
// LDS of the ssim launch: two float32 images of (TH+6) x 72 = 21.9 KB per workgroup; a lane reads 4-byte words at consecutive
// addresses (ds_read_b32: conflict-free at any row stride), and no 8-byte LDS access is on the hot path.
#include "ssim_k.h"
#include "bmc_hip_quality.h"

namespace {

constexpr int QT = 1024;                                   // stats: workgroups of 16 waves, as slot_metrics_kernel
static_assert(BMC_QUALITY_WIN == WIN, "the header's window is the shared tile body's");
constexpr int TH = BMC_QUALITY_TILE_H, TW = BMC_QUALITY_TILE_W;
constexpr int FT = 64;                                     // finish: one wave

struct QSlot {
    const float* gt;
    double* dst;
};
// the slot has a record this window: it is active, has a ground truth and its quality entry has a dst (uniform over the workgroup)
__device__ __forceinline__ bool quality_slot(const bmc_slot_t* table, const bmc_slot_quality_t* quality, int s, QSlot& q) {
    q.gt = gld<const float*>(&table[s].gt);
    q.dst = gld<double*>(&quality[s].dst);
    return (gld<int>(&table[s].flags) & BMC_SLOT_ACTIVE) && gld<const float*>(&table[s].frames) != nullptr && q.gt != nullptr &&
           q.dst != nullptr;
}

// grid (nparts, S): part p owns elements p * QT + tid + j * nparts * QT of the slot's n = 2*gh*gw, as slot_metrics_kernel
__global__ __launch_bounds__(QT) void quality_stats_kernel(const bmc_slot_t* __restrict__ table,
                                                           const bmc_slot_quality_t* __restrict__ quality,
                                                           const float* __restrict__ esr, const float* __restrict__ bic, int gh,
                                                           int gw, double* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ double sh[7][QT / 64];
    const int part = blockIdx.x, nparts = gridDim.x, s = blockIdx.y, tid = threadIdx.x;
    QSlot q;
    if (!quality_slot(table, quality, s, q)) return;
    const int hw = gh * gw, n = 2 * hw;
    const float* const pe = esr + (long long)s * n;
    const float* const pb = bic ? bic + (long long)s * n : nullptr;
    double e0 = 0.0, e1 = 0.0, b0 = 0.0, b1 = 0.0;
    double mx0 = -INFINITY, mx1 = -INFINITY, mn = INFINITY;
#pragma unroll 4
    for (int i = part * QT + tid; i < n; i += nparts * QT) {
        const bool c = i >= hw;
        const double g = (double)gld<float>(q.gt + i);
        const double de = (double)gld<float>(pe + i) - g, se = de * de;
        e0 += c ? 0.0 : se;                                // (an exact zero leaves a non-negative sum as it is)
        e1 += c ? se : 0.0;
        if (pb) {
            const double db = (double)gld<float>(pb + i) - g, sb = db * db;
            b0 += c ? 0.0 : sb;
            b1 += c ? sb : 0.0;
        }
        if (c) mx1 = g > mx1 ? g : mx1;
        else mx0 = g > mx0 ? g : mx0;
        mn = g < mn ? g : mn;
    }
    wave_fold_to(e0, Sum(), sh[0]);
    wave_fold_to(e1, Sum(), sh[1]);
    wave_fold_to(b0, Sum(), sh[2]);
    wave_fold_to(b1, Sum(), sh[3]);
    wave_fold_to(mx0, Max(), sh[4]);
    wave_fold_to(mx1, Max(), sh[5]);
    wave_fold_to(mn, Min(), sh[6]);
    __syncthreads();
    if (tid < BMC_QUALITY_STATS_WORDS) {                   // word `tid` of the part: its waves' values folded in wave order
        constexpr int QW = QT / 64;
        const double r = tid < 4   ? lds_fold<QW>(sh[tid], Sum())
                         : tid < 6 ? lds_fold<QW>(sh[tid], Max())
                         : tid < 7 ? lds_fold<QW>(sh[tid], Min())
                                   : 0.0;
        gst<double>(stats + ((long long)s * nparts + part) * BMC_QUALITY_STATS_WORDS + tid, r);
    }
}

// grid (tiles, images * 2, S); blockIdx.y = image * 2 + channel
__global__ __launch_bounds__(ST) void quality_ssim_kernel(const bmc_slot_t* __restrict__ table,
                                                          const bmc_slot_quality_t* __restrict__ quality,
                                                          const float* __restrict__ esr, const float* __restrict__ bic, int gh,
                                                          int gw, int nparts, double range, int tiles_x,
                                                          const double* __restrict__ stats, double* __restrict__ tiles) {
#pragma clang fp contract(off)      // every float64 operation is rounded on its own, as the contract writes them
    __shared__ SsimTile<TH, TW> t;
    __shared__ double rng[2];
    const int tile = blockIdx.x, ntiles = gridDim.x, ci = blockIdx.y, s = blockIdx.z, tid = threadIdx.x;
    const int c = ci & 1, img = ci >> 1;
    QSlot q;
    if (!quality_slot(table, quality, s, q)) return;
    const int y0 = tile / tiles_x * TH, x0 = tile % tiles_x * TW;      // the tile's first position = its first staged pixel
    if (tid < 64) {                                        // the slot's parts -> max(g[c]) and min(g)
        const double* const o = stats + ((long long)s * nparts + tid) * BMC_QUALITY_STATS_WORDS;
        const double mx = wave_fold(tid < nparts ? gld<double>(o + 4 + c) : -INFINITY, Max());
        const double mn = wave_fold(tid < nparts ? gld<double>(o + 6) : INFINITY, Min());
        if (tid == 0) {
            rng[0] = mx;
            rng[1] = mn;
        }
    }
    const long long plane = (long long)gh * gw;
    t.stage((img ? bic : esr) + ((long long)s * 2 + c) * plane, q.gt + c * plane, y0, x0, gh, gw);     // (its barrier: rng too)
    double* const out = tiles + ((long long)s * 4 + ci) * ntiles + tile;
    const double R = range > 0.0 ? range : rng[0] - rng[1];
    if (R == 0.0) {                                        // (uniform) no defined value: the channel's sum becomes NaN
        if (tid == 0) gst<double>(out, __builtin_nan(""));
        return;
    }
    const double C1 = (0.01 * R) * (0.01 * R), C2 = (0.03 * R) * (0.03 * R);
    const double part = t.sum(y0, x0, gh - AP, gw - AP, C1, C2);
    if (tid == 0) gst<double>(out, part);
}

// grid (images * 2, S), one wave: the record's four words of (slot, image, channel)
__global__ __launch_bounds__(FT) void quality_finish_kernel(const bmc_slot_t* __restrict__ table,
                                                            const bmc_slot_quality_t* __restrict__ quality, int nparts,
                                                            int ntiles, const double* __restrict__ stats,
                                                            const double* __restrict__ tiles) {
#pragma clang fp contract(off)
    __shared__ double sh[3][FT];
    const int ci = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int c = ci & 1;
    QSlot q;
    if (!quality_slot(table, quality, s, q)) return;
    if (tid < nparts) {
        const double* const o = stats + ((long long)s * nparts + tid) * BMC_QUALITY_STATS_WORDS;
        sh[0][tid] = gld<double>(o + ci);
        sh[1][tid] = gld<double>(o + 4 + c);
        sh[2][tid] = gld<double>(o + 6);
    }
    __syncthreads();
    double sse = 0.0, mx = -INFINITY, mn = INFINITY;
    if (tid == 0)
        for (int p = 0; p < nparts; ++p) {                 // in part order
            sse += sh[0][p];
            mx = sh[1][p] > mx ? sh[1][p] : mx;
            mn = sh[2][p] < mn ? sh[2][p] : mn;
        }
    __syncthreads();
    const double* const tp = tiles + ((long long)s * 4 + ci) * ntiles;
    double ssim = 0.0;
    for (int k0 = 0; k0 < ntiles; k0 += FT) {              // the tile partials, FT at a time, in tile order
        if (k0 + tid < ntiles) sh[0][tid] = gld<double>(tp + k0 + tid);
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < FT && k0 + k < ntiles; ++k) ssim += sh[0][k];
        __syncthreads();
    }
    if (tid == 0) {
        double* const o = q.dst + ci * BMC_QUALITY_WORDS;
        gst<double>(o + 0, sse);
        gst<double>(o + 1, mx);
        gst<double>(o + 2, mn);
        gst<double>(o + 3, ssim);
    }
}

}  // namespace

extern "C" int bmc_slot_quality(const bmc_slot_t* table, const bmc_slot_quality_t* quality, int S, const float* esr,
                                const float* bicubic, int gh, int gw, int nparts, double data_range, double* stats, double* tiles,
                                bmc_stream_t s) {
    static_assert(sizeof(bmc_slot_quality_t) == 8, "bmc_slot_quality_t is one pointer");
    BMC_CHECK_ARG(table && quality && esr && stats && tiles && S >= 1 && S <= BMC_MAX_SLOTS, "bmc_slot_quality: bad arguments");
    BMC_CHECK_ARG(gh >= BMC_QUALITY_WIN && gw >= BMC_QUALITY_WIN && 2ll * gh * gw < (1ll << 30),
                  "bmc_slot_quality: images of at least %d x %d and fewer than 2^29 pixels (got %d x %d)", BMC_QUALITY_WIN,
                  BMC_QUALITY_WIN, gh, gw);
    BMC_CHECK_ARG(nparts >= 1 && nparts <= BMC_SLOT_MAX_PARTS, "bmc_slot_quality: 1 <= nparts <= %d (got %d)", BMC_SLOT_MAX_PARTS,
                  nparts);
    BMC_CHECK_ARG(data_range >= 0.0 && data_range <= 1.79769313486231570e308,
                  "bmc_slot_quality: data_range must be 0 (from the ground truth) or a finite positive number");
    BMC_CHECK_ARG(((unsigned long long)quality & 7ull) == 0 && ((unsigned long long)stats & 7ull) == 0 &&
                      ((unsigned long long)tiles & 7ull) == 0 && ((unsigned long long)esr & 3ull) == 0 &&
                      ((unsigned long long)bicubic & 3ull) == 0,
                  "bmc_slot_quality: the quality table, stats and tiles must be 8-byte, the images 4-byte aligned");
    const int tiles_x = (gw - AP + TW - 1) / TW, tiles_y = (gh - AP + TH - 1) / TH, ntiles = tiles_x * tiles_y;
    const int nci = bicubic ? 4 : 2;
    const hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(quality_stats_kernel, dim3(nparts, S), dim3(QT), 0, st, table, quality, esr, bicubic, gh, gw, stats);
    BMC_CHECK_LAUNCH("bmc_slot_quality (stats)");
    hipLaunchKernelGGL(quality_ssim_kernel, dim3(ntiles, nci, S), dim3(ST), 0, st, table, quality, esr, bicubic, gh, gw, nparts,
                       data_range, tiles_x, (const double*)stats, tiles);
    BMC_CHECK_LAUNCH("bmc_slot_quality (ssim)");
    hipLaunchKernelGGL(quality_finish_kernel, dim3(nci, S), dim3(FT), 0, st, table, quality, nparts, ntiles,
                       (const double*)stats, (const double*)tiles);
    BMC_CHECK_LAUNCH("bmc_slot_quality (finish)");
    return 0;
}
