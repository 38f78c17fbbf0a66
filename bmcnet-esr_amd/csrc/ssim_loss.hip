// The structural training loss 1 - mean SSIM and its gradient: the contract, with every summation order, is in
// include/bmc_hip_ssim.h.  The forward's tile launch is slot_quality.hip's ssim launch with a constant data range and one
// partial per (plane, tile): the staging, the separable sums, S and the tree are ssim_k.h's, one body for both.
//
//   bmc_ssim_loss_fwd   tiles   (planes * ntiles)   TH x TW window positions of one plane -> tiles[plane][tile]
//                       finish  (1)                 the partials in index order -> loss = 1 - sum / count, float32
//   bmc_ssim_loss_bwd   grad    (planes * ntiles)   PH x PW PIXELS of one plane: x and y staged with 6 pixels of apron on each
//                                                   side, alpha / beta / gamma of the (PH + 6) x (PW + 6) positions that touch the
//                                                   tile recomputed in double into LDS, then a thread gathers two vertically
//                                                   adjacent pixels from eight rows of 7-term row sums -> dx
// No atomics, no workgroup waits for another, no memset: bit-reproducible.
// LDS: tiles 2 x (TH + 6) x 72 floats = 21.9 KB; grad 2 x 28 x 44 floats + 3 x 22 x 38 doubles = 29.9 KB.
#include "ssim_k.h"
#include "bmc_hip_ssim.h"

namespace {

static_assert(BMC_SSIM_WIN == WIN, "the header's window is the shared tile body's");
constexpr int TH = BMC_SSIM_TILE_H, TW = BMC_SSIM_TILE_W;
constexpr int FT = 256;                                    // finish

constexpr int PH = BMC_SSIM_BWD_TILE_H, PW = BMC_SSIM_BWD_TILE_W;
constexpr int BT = 256;                                    // grad: a thread per column and pair of pixel rows
constexpr int CH = PH + AP, CW = PW + AP;                  // the positions whose windows touch the tile's pixels
constexpr int GH = CH + AP, GW = CW + AP;                  // the pixels those positions read
static_assert(PW == 32 && PH * PW == 2 * BT, "32 columns, two pixel rows per thread");
static_assert(2 * GH * GW * sizeof(float) + 3 * CH * CW * sizeof(double) <= 65536, "static LDS of the grad launch");

// grid (planes * ntiles): workgroup = (plane, tile), tile row-major over the plane's positions
__global__ __launch_bounds__(ST) void ssim_tiles_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        long long y_batch_stride, int C, int h, int w, double range,
                                                        int tiles_x, int ntiles, double* __restrict__ tiles) {
#pragma clang fp contract(off)      // every float64 operation is rounded on its own, as the contract writes them
    __shared__ SsimTile<TH, TW> t;
    const int plane = blockIdx.x / ntiles, tile = blockIdx.x - plane * ntiles;
    const int y0 = tile / tiles_x * TH, x0 = tile % tiles_x * TW;      // the tile's first position = its first staged pixel
    const long long hw = (long long)h * w;
    t.stage(x + plane * hw, y + (plane / C) * y_batch_stride + (plane % C) * hw, y0, x0, h, w);
    const double C1 = (0.01 * range) * (0.01 * range), C2 = (0.03 * range) * (0.03 * range);
    const double part = t.sum(y0, x0, h - AP, w - AP, C1, C2);
    if (threadIdx.x == 0) gst<double>(tiles + blockIdx.x, part);
}

// one workgroup: the partials, FT at a time, in index order
__global__ __launch_bounds__(FT) void ssim_finish_kernel(const double* __restrict__ tiles, int n, double count,
                                                         float* __restrict__ loss) {
#pragma clang fp contract(off)
    __shared__ double sh[FT];
    const int tid = threadIdx.x;
    double sum = 0.0;
    for (int k0 = 0; k0 < n; k0 += FT) {
        if (k0 + tid < n) sh[tid] = gld<double>(tiles + k0 + tid);
        __syncthreads();
        if (tid == 0) {
            const int m = n - k0 < FT ? n - k0 : FT;
            for (int k = 0; k < m; ++k) sum += sh[k];
        }
        __syncthreads();
    }
    if (tid == 0) gst<float>(loss, (float)(1.0 - sum / count));
}

// grid (planes * ntiles): workgroup = (plane, tile), tile row-major over the plane's PIXELS
__global__ __launch_bounds__(BT) void ssim_grad_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       long long y_batch_stride, const float* __restrict__ gloss, int C, int h,
                                                       int w, double range, int tiles_x, int ntiles, double count,
                                                       float* __restrict__ dx) {
#pragma clang fp contract(off)
    __shared__ float lx[GH * GW], ly[GH * GW];
    __shared__ double ca[CH * CW], cb[CH * CW], cg[CH * CW];
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / ntiles, tile = blockIdx.x - plane * ntiles;
    const int ph = h - AP, pw = w - AP;
    const int y0 = tile / tiles_x * PH, x0 = tile % tiles_x * PW;      // the tile's first pixel
    const long long hw = (long long)h * w;
    const float* const X = x + plane * hw;
    const float* const Y = y + (plane / C) * y_batch_stride + (plane % C) * hw;
    for (int k = tid; k < GH * GW; k += BT) {              // staged pixel (r, c) = image pixel (y0 - 6 + r, x0 - 6 + c), or zero
        const int r = k / GW, c = k - r * GW, yy = y0 - AP + r, xx = x0 - AP + c;
        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
        lx[k] = in ? gld<float>(X + (long long)yy * w + xx) : 0.f;
        ly[k] = in ? gld<float>(Y + (long long)yy * w + xx) : 0.f;
    }
    __syncthreads();
    const double C1 = (0.01 * range) * (0.01 * range), C2 = (0.03 * range) * (0.03 * range);
    const double np = (double)(WIN * WIN), cn = np / (double)(WIN * WIN - 1), kc = (2.0 * cn) / np;
    for (int k = tid; k < CH * CW; k += BT) {              // local position (r, c) = position (y0 - 6 + r, x0 - 6 + c)
        const int r = k / CW, c = k - r * CW, p = y0 - AP + r, q = x0 - AP + c;
        double alpha = 0.0, beta = 0.0, gamma = 0.0;       // a position outside the image: exact zeros
        if (p >= 0 && p < ph && q >= 0 && q < pw) {
            Sums v = row_sums(lx + r * GW + c, ly + r * GW + c);
#pragma unroll
            for (int j = 1; j < WIN; ++j) v = plus(v, row_sums(lx + (r + j) * GW + c, ly + (r + j) * GW + c));
            const Terms t = terms(v, C1, C2);
            gamma = -(kc * t.S) / t.B2;                    // x == y: S = A1 / B1 = A2 / B2 = 1, so beta = -gamma and alpha = 0 exactly
            beta = (kc * (t.A1 / t.B1)) / t.B2;
            alpha = (((2.0 * t.uy) / t.B1) * (t.A2 / t.B2) - (2.0 * t.ux * t.S) / t.B1) / np - beta * t.uy - gamma * t.ux;
        }
        ca[k] = alpha;
        cb[k] = beta;
        cg[k] = gamma;
    }
    __syncthreads();
    const int lj = tid & (PW - 1), li = (tid >> 5) * 2;    // pixels (li, lj) and (li + 1, lj) of the tile
    double ra[WIN + 1], rb[WIN + 1], rg[WIN + 1];          // pixel (li, lj) is held by the local positions (li .. li + 6, lj .. lj + 6)
#pragma unroll
    for (int r = 0; r < WIN + 1; ++r) {
        const int o = (li + r) * CW + lj;
        double a = ca[o], b = cb[o], g = cg[o];
#pragma unroll
        for (int k = 1; k < WIN; ++k) {                    // left to right
            a += ca[o + k];
            b += cb[o + k];
            g += cg[o + k];
        }
        ra[r] = a;
        rb[r] = b;
        rg[r] = g;
    }
    const double gl = (double)gld<float>(gloss);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        double sa = ra[d], sb = rb[d], sg = rg[d];
#pragma unroll
        for (int k = 1; k < WIN; ++k) {                    // top to bottom
            sa += ra[d + k];
            sb += rb[d + k];
            sg += rg[d + k];
        }
        const int i = y0 + li + d, j = x0 + lj;
        if (i < h && j < w) {
            const int o = (li + d + AP) * GW + lj + AP;
            const double xv = (double)lx[o], yv = (double)ly[o];
            const double g = (sa + yv * sb) + xv * sg;
            gst<float>(dx + plane * hw + (long long)i * w + j, (float)(-(g / count) * gl));
        }
    }
}

int check(const char* who, const float* x, const float* y, long long y_batch_stride, int B, int C, int h, int w,
          double data_range) {
    BMC_CHECK_ARG(x && y && B >= 1 && C >= 1, "%s: bad arguments", who);
    BMC_CHECK_ARG(h >= WIN && w >= WIN && (long long)B * C * h * w < (1ll << 30),
                  "%s: images of at least %d x %d and fewer than 2^30 elements (got %d x %d x %d x %d)", who, WIN, WIN, B, C, h, w);
    BMC_CHECK_ARG(data_range > 0.0 && data_range <= 1.79769313486231570e308, "%s: data_range must be a finite positive number",
                  who);
    BMC_CHECK_ARG(y_batch_stride >= (long long)C * h * w, "%s: y_batch_stride %lld is below C * h * w = %lld", who,
                  y_batch_stride, (long long)C * h * w);
    return 0;
}

}  // namespace

extern "C" int bmc_ssim_loss_fwd(const float* x, const float* y, long long y_batch_stride, int B, int C, int h, int w,
                                 double data_range, double* tiles, float* loss, bmc_stream_t s) {
    if (check("bmc_ssim_loss_fwd", x, y, y_batch_stride, B, C, h, w, data_range)) return -1;
    BMC_CHECK_ARG(tiles && loss, "bmc_ssim_loss_fwd: bad arguments");
    BMC_CHECK_ARG(((unsigned long long)tiles & 7ull) == 0, "bmc_ssim_loss_fwd: tiles must be 8-byte aligned");
    const int tiles_x = (w - AP + TW - 1) / TW, tiles_y = (h - AP + TH - 1) / TH, ntiles = tiles_x * tiles_y;
    const long long groups = (long long)B * C * ntiles;
    BMC_CHECK_ARG(groups < (1ll << 23), "bmc_ssim_loss_fwd: %lld workgroups, the limit is 2^23", groups);
    const double count = (double)((long long)B * C * (h - AP) * (w - AP));
    const hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(ssim_tiles_kernel, dim3((unsigned)groups), dim3(ST), 0, st, x, y, y_batch_stride, C, h, w, data_range,
                       tiles_x, ntiles, tiles);
    BMC_CHECK_LAUNCH("bmc_ssim_loss_fwd (tiles)");
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(FT), 0, st, (const double*)tiles, (int)groups, count, loss);
    BMC_CHECK_LAUNCH("bmc_ssim_loss_fwd (finish)");
    return 0;
}

extern "C" int bmc_ssim_loss_bwd(const float* x, const float* y, long long y_batch_stride, const float* gloss, int B, int C,
                                 int h, int w, double data_range, float* dx, bmc_stream_t s) {
    if (check("bmc_ssim_loss_bwd", x, y, y_batch_stride, B, C, h, w, data_range)) return -1;
    BMC_CHECK_ARG(gloss && dx, "bmc_ssim_loss_bwd: bad arguments");
    const int tiles_x = (w + PW - 1) / PW, tiles_y = (h + PH - 1) / PH, ntiles = tiles_x * tiles_y;
    const long long groups = (long long)B * C * ntiles;
    BMC_CHECK_ARG(groups < (1ll << 23), "bmc_ssim_loss_bwd: %lld workgroups, the limit is 2^23", groups);
    const double count = (double)((long long)B * C * (h - AP) * (w - AP));
    hipLaunchKernelGGL(ssim_grad_kernel, dim3((unsigned)groups), dim3(BT), 0, (hipStream_t)s, x, y, y_batch_stride, gloss, C, h, w,
                       data_range, tiles_x, ntiles, count, dx);
    BMC_CHECK_LAUNCH("bmc_ssim_loss_bwd");
    return 0;
}
