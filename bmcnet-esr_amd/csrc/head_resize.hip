// Head + bicubic resize + MSE of one window when the ground truth is not of the prediction's size (train.py:227-231, _valid at
// :502-506; EventZoom: 124x224 prediction, 124x222 ground truth), in two launches forward and one backward:
//   pred = pixel_shuffle(x_o, r) + bilinear(base)                       exactly what shuffle_kernel (stream_ops.hip) writes
//   diff = bicubic(pred -> gh x gw) - gt,  loss = mean(diff^2)          taps and summation order of bicubic_fwd_kernel (resize.hip)
//   dlr  = pixel_unshuffle(dpred + (2 gloss / numel) R^T diff)          R^T as a gather, in bicubic_bwd_kernel's order
// The resized value at a ground-truth pixel needs 16 prediction values other threads own: they are RECOMPUTED from x_o / base
// through head_value(), the function the prediction-writing loop calls, so nothing waits for another thread and any gh, gw >= 1
// works.  (The compiler contracts the 16-fold unrolled call differently from the single one: a recomputed value may differ from
// the stored prediction in its last bit.  pred is held to shuffle_kernel's bits, diff and loss to float64 by the 4x rule.)
// The resized prediction and the loss gradient never reach HBM; only diff does, and only when a backward will follow.
// Deterministic: every output element has one writer, the loss is per-block LDS trees summed in index order, no atomics.
// Below the MSE kernels: the same head with a robust loss (L1, Huber, Charbonnier) for a ground truth of either size,
// bmc_head_loss_fwd / _bwd (include/bmc_hip_losses.h) -- the same launch counts, d saved in diff's place.
#include "bmc_common.h"
#include "bmc_hip_losses.h"
#include "cubic_taps.h"

namespace {

constexpr int MAXBLK = 2048;     // = the partials workspace the header asks for

// one element of the head's output; the arithmetic of shuffle_kernel / head_mse_fwd_kernel, expression for expression
__device__ __forceinline__ float head_value(const float* __restrict__ lr, const float* __restrict__ base, long long sb,
                                            long long sc, long long sy, long long sx, int b, int c, int Y, int X, int H, int W,
                                            int r, int CC, float inv) {
    const int y = Y / r, i = Y - y * r, x = X / r, j = X - x * r;
    float v = lr[(((long long)b * H + y) * W + x) * CC + (c * r + i) * r + j];
    float fy = fmaxf((Y + 0.5f) * inv - 0.5f, 0.f), fx = fmaxf((X + 0.5f) * inv - 0.5f, 0.f);
    const int yy0 = (int)fy, xx0 = (int)fx;
    const int yy1 = yy0 + 1 < H ? yy0 + 1 : H - 1, xx1 = xx0 + 1 < W ? xx0 + 1 : W - 1;
    const float ly = fy - yy0, lx = fx - xx0;
    const float* bp = base + b * sb + c * sc;
    const float v00 = bp[yy0 * sy + xx0 * sx], v01 = bp[yy0 * sy + xx1 * sx];
    const float v10 = bp[yy1 * sy + xx0 * sx], v11 = bp[yy1 * sy + xx1 * sx];
    const float top = v00 * (1.f - lx) + v01 * lx, bot = v10 * (1.f - lx) + v11 * lx;
    v += top * (1.f - ly) + bot * ly;
    return v;
}

__global__ void head_resize_mse_fwd_kernel(const float* __restrict__ lr, int B, int C, int H, int W, int r,
                                           const float* __restrict__ base, long long sb, long long sc, long long sy,
                                           long long sx, const float* __restrict__ gt, long long gsb, int gh, int gw, float ry,
                                           float rx, float* __restrict__ hr, float* __restrict__ diff,
                                           float* __restrict__ partials) {
    const int CC = C * r * r, HH = H * r, WW = W * r;
    const float inv = 1.f / r;
    const long long stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    // the prediction: every element once, by the thread that owns it
    const long long npred = (long long)B * C * HH * WW;
    for (long long idx = first; idx < npred; idx += stride) {
        const int X = idx % WW;
        long long t = idx / WW;
        const int Y = t % HH; t /= HH;
        const int c = t % C;
        const int b = (int)(t / C);
        hr[idx] = head_value(lr, base, sb, sc, sy, sx, b, c, Y, X, H, W, r, CC, inv);
    }
    // the resized prediction against the ground truth, one ground-truth element per thread and pass
    const long long per_b = (long long)C * gh * gw, ngt = per_b * B;
    float acc = 0.f;
    for (long long idx = first; idx < ngt; idx += stride) {
        const int X = (int)(idx % gw);
        long long t = idx / gw;
        const int Y = t % gh; t /= gh;
        const int c = t % C;
        const int b = (int)(t / C);
        int iy0, ix0;
        float wy[4], wx[4];
        cubic_taps(Y, ry, iy0, wy);
        cubic_taps(X, rx, ix0, wx);
        int cx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) cx[k] = clampi(ix0 - 1 + k, 0, WW - 1);
        float res = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cy = clampi(iy0 - 1 + j, 0, HH - 1);
            float p[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] = head_value(lr, base, sb, sc, sy, sx, b, c, cy, cx[k], H, W, r, CC, inv);
            // ATen's order: the four taps of a row first, then the rows
            const float rv = p[0] * wx[0] + p[1] * wx[1] + p[2] * wx[2] + p[3] * wx[3];
            res += rv * wy[j];
        }
        const float d = res - gt[(long long)b * gsb + (idx - (long long)b * per_b)];
        if (diff) diff[idx] = d;
        acc += d * d;
    }
    __shared__ float red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// the partials in index order (as mse_finish_kernel of stream_ops.hip)
__global__ void resize_mse_finish_kernel(const float* __restrict__ partials, int n, float scale, float* __restrict__ loss) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = red[0] * scale;
}

__global__ void head_resize_mse_bwd_kernel(const float* __restrict__ dpred, const float* __restrict__ diff,
                                           const float* __restrict__ gloss, int B, int C, int H, int W, int r, int gh, int gw,
                                           float ry, float rx, float* __restrict__ dlr) {
    const int CC = C * r * r, HH = H * r, WW = W * r;
    const long long total = (long long)B * C * HH * WW;
    const float coef = gloss ? 2.f * gloss[0] / (float)((long long)B * C * gh * gw) : 0.f;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int X = idx % WW;
        long long t = idx / WW;
        const int Y = t % HH; t /= HH;
        const int c = t % C;
        const int b = (int)(t / C);
        const int y = Y / r, i = Y - y * r, x = X / r, j = X - x * r;
        float g = dpred ? dpred[idx] : 0.f;
        if (gloss) {
            // every ground-truth pixel whose (clamped) taps touch prediction pixel (Y, X)
            const float* const dp = diff + ((long long)b * C + c) * gh * gw;
            int ylo, yhi, xlo, xhi;
            out_range(Y, ry, gh, ylo, yhi);
            out_range(X, rx, gw, xlo, xhi);
            float acc = 0.f;
            for (int gy = ylo; gy <= yhi; ++gy) {
                const float wy = axis_weight(gy, ry, Y, HH);
                if (wy == 0.f) continue;
                float rs = 0.f;
                for (int gx = xlo; gx <= xhi; ++gx) {
                    const float wx = axis_weight(gx, rx, X, WW);
                    if (wx != 0.f) rs += wx * dp[(long long)gy * gw + gx];
                }
                acc += wy * rs;
            }
            g += coef * acc;
        }
        dlr[(((long long)b * H + y) * W + x) * CC + (c * r + i) * r + j] = g;
    }
}

// ------------------------------------------------------------------ robust losses: L1, Huber, Charbonnier (bmc_head_loss_*)
// One forward and one backward body for every kind and for both ground-truth sizes: KIND picks the pointwise rho / rho',
// RESIZE whether d = bicubic(pred) - gt (the MSE kernels' tap loop and gather) or d = pred - gt (the prediction's own size, as
// head_mse_*_kernel of stream_ops.hip).  The MSE kernels above stay as they are: moving their tap loop into the function below
// changes which product of a tap row the compiler fuses first, and so their last bits.
template <int KIND>
__device__ __forceinline__ float rho(float d, float p) {
    const float a = fabsf(d);
    if constexpr (KIND == BMC_LOSS_L1) return a;
    else if constexpr (KIND == BMC_LOSS_HUBER) return a < p ? 0.5f * d * d : p * (a - 0.5f * p);
    else return sqrtf(d * d + p * p);
}
template <int KIND>
__device__ __forceinline__ float drho(float d, float p) {
    const float sgn = (float)((d > 0.f) - (d < 0.f));       // sign(0) = 0
    if constexpr (KIND == BMC_LOSS_L1) return sgn;
    else if constexpr (KIND == BMC_LOSS_HUBER) return fabsf(d) < p ? d : p * sgn;
    else return d / sqrtf(d * d + p * p);
}

// bicubic(pred -> gh x gw) at ground-truth pixel (Y, X) of plane (b, c), its 16 prediction values recomputed through
// head_value(); taps and summation order of bicubic_fwd_kernel (resize.hip)
__device__ __forceinline__ float resized_value(const float* __restrict__ lr, const float* __restrict__ base, long long sb,
                                               long long sc, long long sy, long long sx, int b, int c, int Y, int X, int H, int W,
                                               int r, int CC, int HH, int WW, float inv, float ry, float rx) {
    int iy0, ix0;
    float wy[4], wx[4];
    cubic_taps(Y, ry, iy0, wy);
    cubic_taps(X, rx, ix0, wx);
    int cx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cx[k] = clampi(ix0 - 1 + k, 0, WW - 1);
    float res = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int cy = clampi(iy0 - 1 + j, 0, HH - 1);
        float p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = head_value(lr, base, sb, sc, sy, sx, b, c, cy, cx[k], H, W, r, CC, inv);
        const float rv = p[0] * wx[0] + p[1] * wx[1] + p[2] * wx[2] + p[3] * wx[3];
        res += rv * wy[j];
    }
    return res;
}

template <int KIND, bool RESIZE>
__global__ void head_loss_fwd_kernel(const float* __restrict__ lr, int B, int C, int H, int W, int r,
                                     const float* __restrict__ base, long long sb, long long sc, long long sy, long long sx,
                                     const float* __restrict__ gt, long long gsb, int gh, int gw, float ry, float rx, float param,
                                     float* __restrict__ hr, float* __restrict__ dsave, float* __restrict__ partials) {
    const int CC = C * r * r, HH = H * r, WW = W * r;
    const float inv = 1.f / r;
    const long long stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per_b = (long long)C * gh * gw;          // = one sample of the prediction where !RESIZE
    float acc = 0.f;
    // the prediction: every element once, by the thread that owns it (and, at the prediction's own size, its loss term)
    const long long npred = (long long)B * C * HH * WW;
    for (long long idx = first; idx < npred; idx += stride) {
        const int X = idx % WW;
        long long t = idx / WW;
        const int Y = t % HH; t /= HH;
        const int c = t % C;
        const int b = (int)(t / C);
        const float v = head_value(lr, base, sb, sc, sy, sx, b, c, Y, X, H, W, r, CC, inv);
        hr[idx] = v;
        if constexpr (!RESIZE) acc += rho<KIND>(v - gt[(long long)b * gsb + (idx - (long long)b * per_b)], param);
    }
    if constexpr (RESIZE) {
        // the resized prediction against the ground truth, one ground-truth element per thread and pass
        const long long ngt = per_b * B;
        for (long long idx = first; idx < ngt; idx += stride) {
            const int X = (int)(idx % gw);
            long long t = idx / gw;
            const int Y = t % gh; t /= gh;
            const int c = t % C;
            const int b = (int)(t / C);
            const float res = resized_value(lr, base, sb, sc, sy, sx, b, c, Y, X, H, W, r, CC, HH, WW, inv, ry, rx);
            const float d = res - gt[(long long)b * gsb + (idx - (long long)b * per_b)];
            if (dsave) dsave[idx] = d;
            acc += rho<KIND>(d, param);
        }
    }
    __shared__ float red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// RESIZE: src = dsave [B,C,gh,gw], gt unused; otherwise src = pred [B,C,rH,rW] and d = pred - gt
template <int KIND, bool RESIZE>
__global__ void head_loss_bwd_kernel(const float* __restrict__ dpred, const float* __restrict__ src, const float* __restrict__ gt,
                                     long long gsb, const float* __restrict__ gloss, int B, int C, int H, int W, int r, int gh,
                                     int gw, float ry, float rx, float param, float* __restrict__ dlr) {
    const int CC = C * r * r, HH = H * r, WW = W * r;
    const long long per_b = (long long)C * HH * WW, total = per_b * B;
    const float coef = gloss ? gloss[0] / (float)((long long)B * C * gh * gw) : 0.f;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int X = idx % WW;
        long long t = idx / WW;
        const int Y = t % HH; t /= HH;
        const int c = t % C;
        const int b = (int)(t / C);
        const int y = Y / r, i = Y - y * r, x = X / r, j = X - x * r;
        float g = dpred ? dpred[idx] : 0.f;
        if (gloss) {
            if constexpr (RESIZE) {
                // every ground-truth pixel whose (clamped) taps touch prediction pixel (Y, X)
                const float* const dp = src + ((long long)b * C + c) * gh * gw;
                int ylo, yhi, xlo, xhi;
                out_range(Y, ry, gh, ylo, yhi);
                out_range(X, rx, gw, xlo, xhi);
                float acc = 0.f;
                for (int gy = ylo; gy <= yhi; ++gy) {
                    const float wy = axis_weight(gy, ry, Y, HH);
                    if (wy == 0.f) continue;
                    float rs = 0.f;
                    for (int gx = xlo; gx <= xhi; ++gx) {
                        const float wx = axis_weight(gx, rx, X, WW);
                        if (wx != 0.f) rs += wx * drho<KIND>(dp[(long long)gy * gw + gx], param);
                    }
                    acc += wy * rs;
                }
                g += coef * acc;
            } else {
                g += coef * drho<KIND>(src[idx] - gt[(long long)b * gsb + (idx - (long long)b * per_b)], param);
            }
        }
        dlr[(((long long)b * H + y) * W + x) * CC + (c * r + i) * r + j] = g;
    }
}

inline int nblk(long long items, int per_block) {
    const long long b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > MAXBLK ? MAXBLK : b));
}

}  // namespace

extern "C" int bmc_head_resize_mse_fwd(const float* xo, int B, int C, int H, int W, int r, const float* base, long long sb,
                                       long long sc, long long sy, long long sx, const float* gt, long long gt_batch_stride,
                                       int gh, int gw, float* pred, float* diff, float* partials, float* loss, bmc_stream_t s) {
    BMC_CHECK_ARG(xo && base && gt && pred && partials && loss, "bmc_head_resize_mse_fwd: null pointer");
    BMC_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && r > 0 && gh > 0 && gw > 0,
                  "bmc_head_resize_mse_fwd: B=%d C=%d H=%d W=%d r=%d gh=%d gw=%d must be positive", B, C, H, W, r, gh, gw);
    BMC_CHECK_ARG((long long)H * r <= 0x7fffffffLL && (long long)W * r <= 0x7fffffffLL,
                  "bmc_head_resize_mse_fwd: prediction %lld x %lld too large", (long long)H * r, (long long)W * r);
    const long long npred = (long long)B * C * H * W * r * r, ngt = (long long)B * C * gh * gw;
    // a ground-truth element costs 16 head values: a quarter of the elements per thread of the prediction's side
    const int nbp = nblk(npred, 256 * 4), nbg = nblk(ngt, 256);
    const int nb = nbp > nbg ? nbp : nbg;    // <= 2048 partials
    hipLaunchKernelGGL(head_resize_mse_fwd_kernel, dim3(nb), dim3(256), 0, (hipStream_t)s, xo, B, C, H, W, r, base, sb, sc, sy,
                       sx, gt, gt_batch_stride, gh, gw, (float)(H * r) / (float)gh, (float)(W * r) / (float)gw, pred, diff,
                       partials);
    hipLaunchKernelGGL(resize_mse_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, partials, nb, 1.f / (float)ngt, loss);
    BMC_CHECK_LAUNCH("bmc_head_resize_mse_fwd");
    return 0;
}

extern "C" int bmc_head_resize_mse_bwd(const float* dpred, const float* diff, const float* gloss, int B, int C, int H, int W,
                                       int r, int gh, int gw, float* dlr, bmc_stream_t s) {
    BMC_CHECK_ARG(dlr && (dpred || gloss) && (!gloss || diff), "bmc_head_resize_mse_bwd: bad arguments");
    BMC_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && r > 0 && gh > 0 && gw > 0,
                  "bmc_head_resize_mse_bwd: B=%d C=%d H=%d W=%d r=%d gh=%d gw=%d must be positive", B, C, H, W, r, gh, gw);
    BMC_CHECK_ARG((long long)H * r <= 0x7fffffffLL && (long long)W * r <= 0x7fffffffLL,
                  "bmc_head_resize_mse_bwd: prediction %lld x %lld too large", (long long)H * r, (long long)W * r);
    const long long n = (long long)B * C * H * W * r * r;
    hipLaunchKernelGGL(head_resize_mse_bwd_kernel, dim3(nblk(n, gloss ? 256 : 256 * 4)), dim3(256), 0, (hipStream_t)s, dpred,
                       diff, gloss, B, C, H, W, r, gh, gw, (float)(H * r) / (float)gh, (float)(W * r) / (float)gw, dlr);
    BMC_CHECK_LAUNCH("bmc_head_resize_mse_bwd");
    return 0;
}

namespace {

// kind known, and a finite positive parameter where the kind has one
inline bool loss_kind_ok(int kind) { return kind == BMC_LOSS_L1 || kind == BMC_LOSS_HUBER || kind == BMC_LOSS_CHARBONNIER; }
inline bool loss_param_ok(int kind, float param) { return kind == BMC_LOSS_L1 || (param > 0.f && param <= 3.402823466e38f); }

// the instantiation of KERNEL for a runtime (kind, resize)
#define BMC_LOSS_DISPATCH(KERNEL, kind, resize, ...)                                                           \
    do {                                                                                                        \
        if ((kind) == BMC_LOSS_L1) {                                                                            \
            if (resize) hipLaunchKernelGGL((KERNEL<BMC_LOSS_L1, true>), __VA_ARGS__);                           \
            else hipLaunchKernelGGL((KERNEL<BMC_LOSS_L1, false>), __VA_ARGS__);                                 \
        } else if ((kind) == BMC_LOSS_HUBER) {                                                                  \
            if (resize) hipLaunchKernelGGL((KERNEL<BMC_LOSS_HUBER, true>), __VA_ARGS__);                        \
            else hipLaunchKernelGGL((KERNEL<BMC_LOSS_HUBER, false>), __VA_ARGS__);                              \
        } else {                                                                                                \
            if (resize) hipLaunchKernelGGL((KERNEL<BMC_LOSS_CHARBONNIER, true>), __VA_ARGS__);                  \
            else hipLaunchKernelGGL((KERNEL<BMC_LOSS_CHARBONNIER, false>), __VA_ARGS__);                        \
        }                                                                                                       \
    } while (0)

}  // namespace

extern "C" int bmc_head_loss_fwd(const float* xo, int B, int C, int H, int W, int r, const float* base, long long sb, long long sc,
                                 long long sy, long long sx, const float* gt, long long gt_batch_stride, int gh, int gw,
                                 float* pred, float* dsave, float* partials, float* loss, int kind, float param, bmc_stream_t s) {
    BMC_CHECK_ARG(xo && base && gt && pred && partials && loss, "bmc_head_loss_fwd: null pointer");
    BMC_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && r > 0 && gh > 0 && gw > 0,
                  "bmc_head_loss_fwd: B=%d C=%d H=%d W=%d r=%d gh=%d gw=%d must be positive", B, C, H, W, r, gh, gw);
    BMC_CHECK_ARG(loss_kind_ok(kind), "bmc_head_loss_fwd: unknown loss kind %d", kind);
    BMC_CHECK_ARG(loss_param_ok(kind, param), "bmc_head_loss_fwd: param %g of loss kind %d must be finite and positive",
                  (double)param, kind);
    BMC_CHECK_ARG((long long)H * r <= 0x7fffffffLL && (long long)W * r <= 0x7fffffffLL,
                  "bmc_head_loss_fwd: prediction %lld x %lld too large", (long long)H * r, (long long)W * r);
    const bool resize = (long long)gh != (long long)H * r || (long long)gw != (long long)W * r;
    const long long npred = (long long)B * C * H * W * r * r, ngt = (long long)B * C * gh * gw;
    // as the MSE entry points: 4 prediction elements per thread, and where it is resampled one ground-truth element (16 head values)
    const int nbp = nblk(npred, 256 * 4), nbg = resize ? nblk(ngt, 256) : 1;
    const int nb = nbp > nbg ? nbp : nbg;    // <= 2048 partials
    BMC_LOSS_DISPATCH(head_loss_fwd_kernel, kind, resize, dim3(nb), dim3(256), 0, (hipStream_t)s, xo, B, C, H, W, r, base, sb, sc,
                      sy, sx, gt, gt_batch_stride, gh, gw, (float)(H * r) / (float)gh, (float)(W * r) / (float)gw, param, pred,
                      dsave, partials);
    hipLaunchKernelGGL(resize_mse_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, partials, nb, 1.f / (float)ngt, loss);
    BMC_CHECK_LAUNCH("bmc_head_loss_fwd");
    return 0;
}

extern "C" int bmc_head_loss_bwd(const float* dpred, const float* dsave, const float* pred, const float* gt,
                                 long long gt_batch_stride, const float* gloss, int B, int C, int H, int W, int r, int gh, int gw,
                                 int kind, float param, float* dlr, bmc_stream_t s) {
    BMC_CHECK_ARG(dlr && (dpred || gloss), "bmc_head_loss_bwd: bad arguments (dlr, and dpred or gloss)");
    BMC_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && r > 0 && gh > 0 && gw > 0,
                  "bmc_head_loss_bwd: B=%d C=%d H=%d W=%d r=%d gh=%d gw=%d must be positive", B, C, H, W, r, gh, gw);
    BMC_CHECK_ARG(loss_kind_ok(kind), "bmc_head_loss_bwd: unknown loss kind %d", kind);
    BMC_CHECK_ARG(loss_param_ok(kind, param), "bmc_head_loss_bwd: param %g of loss kind %d must be finite and positive",
                  (double)param, kind);
    BMC_CHECK_ARG((long long)H * r <= 0x7fffffffLL && (long long)W * r <= 0x7fffffffLL,
                  "bmc_head_loss_bwd: prediction %lld x %lld too large", (long long)H * r, (long long)W * r);
    const bool resize = (long long)gh != (long long)H * r || (long long)gw != (long long)W * r;
    BMC_CHECK_ARG(!gloss || (resize ? dsave != nullptr : (pred && gt)),
                  "bmc_head_loss_bwd: gloss needs %s", resize ? "dsave (the ground truth has another size)" : "pred and gt");
    const long long n = (long long)B * C * H * W * r * r;
    const int nb = nblk(n, gloss && resize ? 256 : 256 * 4);
    BMC_LOSS_DISPATCH(head_loss_bwd_kernel, kind, resize, dim3(nb), dim3(256), 0, (hipStream_t)s, dpred, resize ? dsave : pred, gt,
                      gt_batch_stride, gloss, B, C, H, W, r, gh, gw, (float)(H * r) / (float)gh, (float)(W * r) / (float)gw, param,
                      dlr);
    BMC_CHECK_LAUNCH("bmc_head_loss_bwd");
    return 0;
}
