// Kernel-argument block shared by the convolution kernels (conv.hip: fp32 MFMA; conv_bf.hip: bf16-plane MFMA).
#pragma once
#include "bmc_common.h"

struct ConvK {
    int nsrc;
    SrcDev src[BMC_MAX_SRC];
    const void* w;     // packed weights: fp32 [S][Coutpad][16] or bf16 planes [S][NP][Coutpad][16] (conv_bf.hip)
    const float* bias;
    long long w_group_stride;
    int bias_group_stride;
    int batch_per_group;
    float* out;
    long long out_batch_stride;
    int out_pix_stride;
    int B, H, W, Cout, Coutpad;
    int relu;
    SrcDev residual;
    SrcDev mask;
    int accumulate;
    int tiles_x, tiles_y, ntn, nchunks, ntiles;
    // batch segment (bmc_conv_args_t::seg_b): launch images b >= seg_b of an operand start seg_delta floats past where its
    // descriptor puts them (the second tensor of the operand); all deltas are 0 in a launch without one, so `b >= seg_b ? delta : 0`
    // needs no "is there a segment" test.  Launch-level fields, not SrcDev's: the descriptor stays 32 bytes for every other kernel.
    int seg_b;
    long long seg_delta[BMC_MAX_SRC];
    long long res_seg_delta, mask_seg_delta;
};
// The kernels read the segment from an LDS table of BMC_SEG_TAB long longs, where they use it (once per image and operand): the
// sources' deltas by source number, then the residual's, the mask's, and seg_b.  Read from the argument block, the five scalars of
// the epilogue operands were loaded at the kernel's entry and spilled across the chunk loops (wino4_conv_kernel: 109 -> 122 SGPRs).
constexpr int BMC_SEG_RES = BMC_MAX_SRC, BMC_SEG_MASK = BMC_MAX_SRC + 1, BMC_SEG_B = BMC_MAX_SRC + 2, BMC_SEG_TAB = BMC_MAX_SRC + 3;
// Kernel prologue, beside BMC_LOAD_SRC_TABLE (and a macro for the same reason).  Threads 32.. : no lane shared with that copy.
#define BMC_LOAD_SEG_TABLE(segtab, a, tid)                                       \
    do {                                                                         \
        _Pragma("unroll") for (int i_ = 0; i_ < BMC_MAX_SRC; ++i_)               \
            if ((tid) == 32 + i_) (segtab)[i_] = (a).seg_delta[i_];              \
        if ((tid) == 32 + BMC_SEG_RES) (segtab)[BMC_SEG_RES] = (a).res_seg_delta;    \
        if ((tid) == 32 + BMC_SEG_MASK) (segtab)[BMC_SEG_MASK] = (a).mask_seg_delta; \
        if ((tid) == 32 + BMC_SEG_B) (segtab)[BMC_SEG_B] = (a).seg_b;            \
    } while (0)
// floats to add to the base of launch image b of operand `which` (b and the table are wave-uniform: the result is scalar)
__device__ __forceinline__ long long seg_off(const long long* segtab, int which, int b) {
    const unsigned long long dv = (unsigned long long)segtab[which];
    const int seg_b = __builtin_amdgcn_readfirstlane((int)segtab[BMC_SEG_B]);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)dv), hi = __builtin_amdgcn_readfirstlane((unsigned)(dv >> 32));
    return b >= seg_b ? (long long)(((unsigned long long)hi << 32) | lo) : 0ll;
}
// the same left in vector registers, for a caller that makes the whole address there and takes its first lane afterwards
__device__ __forceinline__ long long seg_off_v(const long long* segtab, int which, int b) {
    return b >= (int)segtab[BMC_SEG_B] ? segtab[which] : 0ll;
}
static inline bool conv_has_segment(const ConvK& k) { return k.seg_b != 0; }

// Kernel prologue: accumulator start values for the BN channels of a tile -- the bias when it is the same for every tile of
// the launch (one weight group, one channel tile: the usual case; returns true then), zeros otherwise.  A tile's
// accumulators are (re)initialised with LDS reads straight into the accumulator registers: that replaces the v_movs, the
// bias adds and the bias loads of the epilogue, and VALU instructions issued beside the other workgroups' MFMAs cost
// 20-30 cycles each (in-kernel stamps).  The caller's barrier publishes the values.
__device__ __forceinline__ bool bias_start_values(float* init_lds, const ConvK& a, int BN, int tid) {
    const bool bias_pre = a.bias != nullptr && a.batch_per_group >= a.B && a.ntn == 1;
    if (tid < BN) init_lds[tid] = (bias_pre && tid < a.Cout) ? a.bias[tid] : 0.f;
    return bias_pre;
}

// conv_bf.hip: launch the bf16-plane kernel (planes = 1: bf16 operands; 3: fp32 operands split into three bf16 planes,
// six plane products -- fp32-equivalent result) for an already validated argument block.
int bmc_conv_bf_launch(const ConvK& k, int taps, int BN, int TH, int planes, int cus, hipStream_t st);

// conv1.hip: 1x1 convolution on the 16x16x4 fp32 MFMA with LDS-DMA operand rings (large problems).  Returns 1 if it
// launched the problem, 0 if it is left to conv.hip's kernel.
int bmc_conv1_launch(ConvK k, int cus, hipStream_t st);

// conv1p.hip: the same for Coutpad % 128 == 0 and K = 128 / 256 with the weights resident in registers (tried first by
// bmc_conv1_launch).  Returns 1 if it launched the problem.
int bmc_conv1p_launch(ConvK k, int cus, hipStream_t st);

// wino.hip: 3x3 convolution through the Winograd transform F(2x2, 3x3) on the fp32 MFMA (math = BMC_MATH_FP32_WINO; weights from
// bmc_pack_weight_wino).  Returns 0, or < 0 with the error text set.
int bmc_conv_wino_launch(ConvK k, int cus, hipStream_t st);
// wino4.hip: the same through F(4x4, 3x3) (math = BMC_MATH_FP32_WINO4; weights from bmc_pack_weight_wino4; images at least 17
// pixels wide, 32-bit pixel offsets).  Returns 0, or < 0 with the error text set.
int bmc_conv_wino4_launch(ConvK k, int cus, hipStream_t st);
