// The SSIM tile arithmetic (internal), shared by the training loss (ssim_loss.hip) and the slots' quality record
// (slot_quality.hip): 7x7 uniform window, sample covariance, float64 on float32 pixels.  Every summation order that
// include/bmc_hip_ssim.h and include/bmc_hip_quality.h promise is written here once, so the two launches give the same bits
// for the same pixels and range by construction (tests/test_gpu_ssim_tiles_shared.py).
#pragma once
#include "wave_k.h"

namespace {

constexpr int WIN = 7, AP = WIN - 1;
constexpr int ST = 256, SW = ST / 64;                      // a tile's workgroup: 4 waves, each a strip of TH / 4 position rows
constexpr int LS = 72;                                     // floats between staged rows

// the five sums of a window position (or of one of its rows)
struct Sums {
    double x, y, xx, yy, xy;
};
__device__ __forceinline__ Sums plus(const Sums& a, const Sums& b) {
    return Sums{a.x + b.x, a.y + b.y, a.xx + b.xx, a.yy + b.yy, a.xy + b.xy};
}
// the sums of the seven pixels at a[0..6], g[0..6], left to right
__device__ __forceinline__ Sums row_sums(const float* a, const float* g) {
#pragma clang fp contract(off)
    const double a0 = (double)a[0], g0 = (double)g[0];
    Sums t{a0, g0, a0 * a0, g0 * g0, a0 * g0};
#pragma unroll
    for (int k = 1; k < WIN; ++k) {
        const double ak = (double)a[k], gk = (double)g[k];
        t = plus(t, Sums{ak, gk, ak * ak, gk * gk, ak * gk});
    }
    return t;
}

struct Terms {
    double ux, uy, A1, A2, B1, B2, D, S;
};
__device__ __forceinline__ Terms terms(const Sums& v, double C1, double C2) {
#pragma clang fp contract(off)
    const double np = (double)(WIN * WIN), nm1 = (double)(WIN * WIN - 1);
    Terms t;
    t.ux = v.x / np;
    t.uy = v.y / np;
    const double vx = (v.xx - v.x * v.x / np) / nm1, vy = (v.yy - v.y * v.y / np) / nm1;
    const double vxy = (v.xy - v.x * v.y / np) / nm1;
    t.A1 = 2.0 * t.ux * t.uy + C1;
    t.A2 = 2.0 * vxy + C2;
    t.B1 = t.ux * t.ux + t.uy * t.uy + C1;
    t.B2 = vx + vy + C2;
    t.D = t.B1 * t.B2;
    t.S = (t.A1 * t.A2) / t.D;
    return t;
}

// TH x TW window positions of one plane, summed by one workgroup of ST threads; a __shared__ object (2 x (TH + 6) x LS floats).
// A lane owns a column of positions: it forms the row sums of the staged rows of its wave's strip one after another and keeps
// the last seven in registers (doubles for a tile would not fit in LDS), reading 4-byte words at consecutive addresses.
template <int TH, int TW>
struct SsimTile {
    static constexpr int STRIP = TH / SW, LH = TH + AP, LW = TW + AP;
    static_assert(TW == 64 && TH % SW == 0 && LS >= LW, "a lane per column of positions, whole strips");
    static_assert(2 * LH * LS * sizeof(float) + 64 <= 65536, "static LDS of a tile launch");
    float la[LH * LS], lg[LH * LS];
    double wsum[SW];

    // the tile's pixels of the h x w planes A and G, from the tile's first position (y0, x0) = its first staged pixel; pixels
    // outside the image are zeros, read by positions outside it only.  Ends with the workgroup's barrier.
    __device__ __forceinline__ void stage(const float* A, const float* G, int y0, int x0, int h, int w) {
        for (int k = threadIdx.x; k < LH * LW; k += ST) {
            const int r = k / LW, col = k - r * LW, yy = y0 + r, xx = x0 + col;
            const bool in = yy < h && xx < w;
            la[r * LS + col] = in ? gld<float>(A + (long long)yy * w + xx) : 0.f;
            lg[r * LS + col] = in ? gld<float>(G + (long long)yy * w + xx) : 0.f;
        }
        __syncthreads();
    }

    // S of the tile's positions inside the ph x pw positions of the image (an exact 0.0 for the others), folded over the lanes
    // in a fixed tree and over the waves as ((w0 + w1) + w2) + w3 (wave_k.h's block_fold): the partial, on thread 0.  Holds a
    // barrier.
    __device__ __forceinline__ double sum(int y0, int x0, int ph, int pw, double C1, double C2) {
#pragma clang fp contract(off)      // every float64 operation is rounded on its own, as the contracts write them
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const bool col_in = x0 + lane < pw;
        Sums hs[WIN];                                      // the row sums of the last seven staged rows (static indices below)
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < STRIP + AP; ++r) {
            hs[r % WIN] = row_sums(la + (wave * STRIP + r) * LS + lane, lg + (wave * STRIP + r) * LS + lane);
            if (r >= AP) {                                 // position row r - 6 of the strip: its seven rows, top to bottom
                Sums v = hs[(r - AP) % WIN];
#pragma unroll
                for (int k = 1; k < WIN; ++k) v = plus(v, hs[(r - AP + k) % WIN]);
                const double S = terms(v, C1, C2).S;
                const bool in = col_in && y0 + wave * STRIP + (r - AP) < ph;
                acc += in ? S : 0.0;
            }
        }
        return block_fold<SW>(acc, Sum(), wsum);
    }
};

}  // namespace
