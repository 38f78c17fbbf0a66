// ATen's bicubic taps (F.interpolate(..., mode='bicubic', align_corners=False)), shared by the loss-side resize (resize.hip)
// and the per-slot inference metrics (slots.hip).  Per axis: scale = in / out (float), src = fma(scale, dst + 0.5, -0.5) (not
// clamped), i0 = floor(src), t = src - i0, taps i0-1 .. i0+2 with the cubic-convolution weights for A = -0.75; the caller clamps
// the tap indices to [0, in-1].
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr float CUBIC_A = -0.75f;

__device__ __forceinline__ void cubic_taps(int dst, float scale, int& i0, float (&w)[4]) {
    const float src = fmaf(scale, (float)dst + 0.5f, -0.5f);
    const float fl = floorf(src);
    const float t = src - fl;
    i0 = (int)fl;
    auto c1 = [](float v) { return ((CUBIC_A + 2.f) * v - (CUBIC_A + 3.f)) * v * v + 1.f; };                     // |v| <= 1
    auto c2 = [](float v) { return ((CUBIC_A * v - 5.f * CUBIC_A) * v + 8.f * CUBIC_A) * v - 4.f * CUBIC_A; };   // 1 < |v| < 2
    w[0] = c2(t + 1.f); w[1] = c1(t); w[2] = c1(1.f - t); w[3] = c2(2.f - t);
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The transposed operator as a gather (resize.hip's backward, head_resize.hip's backward):
// weight with which output index `dst` reads input index `src_i` along one axis (sum over its clamped taps)
__device__ __forceinline__ float axis_weight(int dst, float scale, int src_i, int n_in) {
    int i0;
    float w[4];
    cubic_taps(dst, scale, i0, w);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (clampi(i0 - 1 + k, 0, n_in - 1) == src_i) s += w[k];
    return s;
}
// conservative range of output indices whose taps can touch input index i (the exact test is axis_weight != 0)
__device__ __forceinline__ void out_range(int i, float scale, int n_out, int& lo, int& hi) {
    const float inv = 1.f / scale;
    lo = (int)floorf(((float)i - 2.f + 0.5f) * inv - 0.5f) - 1;
    hi = (int)ceilf(((float)i + 2.f + 0.5f) * inv - 0.5f) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_out - 1 ? n_out - 1 : hi;
}

}  // namespace
