// Fused "centre" chain of the BIE block on the fp32 matrix cores (v_mfma_f32_32x32x2_f32):
//
//   forward  (models/submodules.py:63-64, 127-140):   z = convf(cat[s0, s1]) + b_f            1x1, 2C -> C
//                                                      yhat = (z - mean_c z) * rstd            LayerNorm2d, eps inside the sqrt
//                                                      centre = clustering(yhat*gamma + beta)  1x1, C -> C
//   backward (autograd of the same, LayerNormFunction.backward :141-154):
//                                                      dy = W_c^T dcentre;  dz = LN'(dy);  d s0 += W_f[:, :C]^T dz;  d s1 = W_f[:, C:]^T dz
//
// One launch per direction instead of conv -> LayerNorm -> conv (forward) and dgrad -> LayerNorm-backward -> 3 dgrads
// (backward): z, y = LN(z) and dy never travel to HBM.  What makes the fusion cheap on this machine: the 32x32x2 fp32
// MFMA takes ONE register per operand per lane, and its result layout (rows = channels in the 16 registers, columns =
// pixels on the lanes, lane half h owning rows 4h..4h+3 of every 8) is exactly the B-operand layout of a following
// MFMA that sums over the channel index, with the k order (c, c + 4) that the weight fragment reads (4 consecutive k
// at offset 4h) already use.  So the second GEMM of the chain takes its pixel operand straight from the first one's
// accumulators: no LDS round trip, no shuffles.  The per-pixel LayerNorm reductions are in-lane sums over 64
// registers plus one exchange between lanes l and l + 32.
//
// Workgroup = 4 waves = 8x16 pixels; wave = 2 rows x 16 pixels = 32 pixels x ALL C channels (NU = C/32 MFMA tiles), so
// a pixel's channels live in two lanes of one wave.  K is walked in 16-channel steps; a step's [C][16] weight slice
// streams through a double-buffered LDS image (loaded two steps ahead, one barrier per step), input pixels of the
// first GEMM are staged through LDS like in conv.hip (coalesced 16-byte loads, conflict-free ds_read_b128).
// Persistent workgroups (at C = 128 one per CU: two 64-register result tiles + operands per lane do not fit the 256
// registers that two waves per SIMD would leave), load pipeline running across tile boundaries, XCD-contiguous tile ranges.
//
// Backward works on PAIRS of tiles (batch b and b + n, the two polarity halves of the twin layout) so that the two
// contributions to the shared stream's gradient d s0[b] are summed in registers: no read-modify-write of d s0.
// Weight gradients stay with the pixel-reduction GEMM (pgemm.hip): it reads (dcentre, yhat) and (dz, s0, s1); the
// LayerNorm affine gradients follow algebraically from its results (bmc_chain_affine_grads below).
#include "bmc_common.h"
#include "dma_ring.h"
#include "tile_walk.h"

namespace {

constexpr int CK = BMC_CK;
constexpr int TW = 16, TH = 4, NPX = TW * TH;      // workgroup tile: 4 rows x 16 pixels, one row per wave
__device__ __attribute__((aligned(16))) const float g_zero4c[4] = {0.f, 0.f, 0.f, 0.f};

struct ChainK {
    SrcDev src[2];        // fwd: s0, s1 (C channels each, with their batch maps); bwd: src[0] = dcentre (C channels)
    const float* w;       // weight stream of one unit, slices of [C][16] floats in consumption order
    const float* vec[4];  // fwd: b_f, b_c, gamma, beta;  bwd: -, -, gamma, -
    float eps;
    float* out0;          // fwd: yhat   [B][H][W][C]     bwd: dz    [2n][H][W][C]
    float* out1;          // fwd: centre [B][H][W][C]     bwd: d s1  [2n][H][W][C]  (written at batch (bb + n) % 2n)
    float* out2;          // fwd: rstd   [B][H][W]        bwd: d s0  [n][H][W][C]
    const float* in0;     // bwd: yhat
    const float* in1;     // bwd: rstd
    SrcDev res;           // bwd: term added to d s0 (upstream gradient of the skip connection), or ptr == nullptr
    int nb;               // fwd: launch batches B; bwd: n (pairs)
    int n;                // bwd: batch distance of the two halves
    int H, W, tiles_x, tiles_y, nunits;
};

// Two (or more) independent workgroups per CU hide each other's LayerNorm / epilogue / barrier phases (a first version
// with 32x32x2 MFMAs needed 128 accumulator registers per lane for its two result tiles = one workgroup per CU, and ran
// its matrix pipes only 60 % busy: every non-MFMA instruction of the single wave per SIMD was exposed).  Both operand
// streams run through LDS rings filled by LDS-DMA several steps ahead -- X chunks (64 px x 16 ch = 4 KB, from HBM) DX
// chunks ahead, weight slices (C x 16, from L2) DW steps ahead.  Roles by wave (a wave's vmcnt completes in order: a
// wave waiting for a weight slice would wait for its younger X chunks too): waves 0-1 fill the X ring, waves 2-3 the W
// ring; all four compute.  Rows are 64 B without padding; the 16-byte quads of a row are XOR-swizzled with
// SWZ[(row >> 2) & 3] on the DMA's SOURCE address and on the fragment reads (conflict-free ds_read_b128 for the
// 16-row x 4-quad fragment shape), the LDS destination of a DMA stays lane-linear.
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// PAIR (forward only): a unit is the pixel tile of batch b TOGETHER with the same tile of batch b + n (n = B / 2) of a
// launch whose s0 maps both to one image (the twin layout: s0 = xs with mod = n).  W_f[:, :C] s0 + b_f is then the same
// bits for both, so it is computed once and kept in Rz: 5 NR steps per pair instead of 6 NR for two units, and the shared
// s0 chunks are fetched once.  Each accumulator's MFMA chain is instruction for instruction that of the unpaired kernel.
// 16-byte store to global memory (the address went through integers: without the address space it would be a flat store)
__device__ __forceinline__ void stg16(float* p, f32x4 v) {
    *(__attribute__((address_space(1))) f32x4*)(unsigned long long)p = v;
}

template <int NT, bool BWD, bool PAIR = false>
__global__ __launch_bounds__(256, 2) void chain_kernel(const ChainK a) {
    static_assert(!(BWD && PAIR), "the backward always walks pairs");
    constexpr int C = 16 * NT;
    constexpr int NR = NT;                        // steps of one register-operand GEMM (K = C, 16 per step)
    constexpr int NS = (BWD || PAIR) ? 5 * NR : 3 * NR;     // steps per unit
    constexpr int NSEG = PAIR ? 3 : 2;            // X segments of C channels per unit
    constexpr int NXC = NSEG * NR;                // X chunks per unit
    constexpr int DX = 6, NXR = 8, DW = 3, NWR = 5;
    constexpr int XSLOT = NPX * CK, WSLOT = C * CK;          // floats per ring slot
    constexpr int NDX = NPX / 32;                 // DMA instructions (16 rows = 1 KB each) per X wave and chunk
    constexpr int NDW = (C + 31) / 32;            // ... per W wave and slice
    // The per-channel vectors sit at the START of LDS: every read of them is then one lane-dependent base register plus an
    // immediate offset.  Behind the rings (past 64 KB, beyond the reach of a ds_read's offset field) the compiler kept one
    // address register per vector and channel tile alive across the whole unit loop, ~30 at C = 128.  The rings follow 16-byte
    // aligned: shifting every address of a ds_read_b128 or a DMA image by one multiple of 16 B rotates the banks and changes
    // no conflict.
    constexpr int HEAD = 5 * C + 2 * 8;                      // floats
    __shared__ __attribute__((aligned(16))) float lds[HEAD + NXR * XSLOT + NWR * WSLOT];
    float* const img = lds;                                  // [0] b_f | 0   [1] b_c | 0   [2] gamma   [3] beta   [4] zeros
    SrcDev* const tab = reinterpret_cast<SrcDev*>(lds + 5 * C);
    float* const Xb = lds + HEAD;
    float* const Wb = lds + HEAD + NXR * XSLOT;
    const unsigned xb_lds = lds_addr(Xb), wb_lds = lds_addr(Wb);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lp = lane & 15, lg = lane >> 4;     // pixel of the wave's row / channel quad: D rows 4*lg .. 4*lg+3
    if (tid < 2) tab[tid] = a.src[tid];
    for (int i = tid; i < 5 * C; i += 256) {
        const int k = i / C, c = i - k * C;
        img[i] = (k < 4 && a.vec[k]) ? a.vec[k][c] : 0.f;
    }
    __syncthreads();

    const TileWalk tw = tile_walk(a.nunits);      // persistent workgroups; a unit = one 8 x 16 pixel tile, all channels
    const int t_first = tw.first, t_hi = tw.hi, t_stride = tw.stride, my_units = tw.count;
    if (my_units == 0) return;
    const int total_steps = my_units * NS, total_xchunks = my_units * NXC;

    using UnitIt = Tile3;         // (no channel tiles: nt = 0)
    auto decode = [&](int t) { return tile_decode(t, 1, a.tiles_x, a.tiles_y); };

    // ---- X ring loader (waves 0-1): chunks of 16 channels in consumption order; a unit has NSEG segments of C channels
    //      (fwd: s0 then s1 at batch b; paired fwd: s0 at b, s1 at b, s1 at b + n; bwd: dcentre at batch b then at
    //      batch b + n).  Instruction i of X wave w covers the
    //      16 tile pixels [(NDX w + i) * 16, +16) = tile row NDX w + i, 4 lanes per pixel row; lane (pixel p, position q')
    //      fetches quad q' ^ swz(p).  Pixels outside the image re-read the clamped edge pixel: their columns of the result
    //      are never stored, and a pixel's column never mixes with another's.
    const bool xrole = wave < 2;
    int xl_unit = t_first, xl_seg = 0, c_in = 0, xl_cnt = 0;
    UnitIt xl_it = decode(t_first);
    const float* sbase = nullptr;
    int xpixq[NDX];               // pixel index of this lane's row per instruction (tile-dependent)
    unsigned xvoff[NDX];          // byte offset from the segment's batch pointer (segment-dependent: pixel stride)
    const int xq = ((lane & 3) ^ swz(lane >> 2)) * 4;         // row index within the instruction = lane / 4
    auto seg_select = [&]() {
        const SrcDev S = tab[BWD ? 0 : PAIR ? (xl_seg ? 1 : 0) : xl_seg];
        sbase = src_batch_ptr(S, BWD ? xl_it.b + xl_seg * a.n : (PAIR && xl_seg == 2) ? xl_it.b + a.n : xl_it.b);
#pragma unroll
        for (int i = 0; i < NDX; ++i) xvoff[i] = (unsigned)(xpixq[i] * S.pix_stride + xq) * 4u;
    };
    auto xl_setup = [&]() {
        const int y0 = xl_it.ty * TH, x0 = xl_it.tx * TW;
#pragma unroll
        for (int i = 0; i < NDX; ++i) {
            int y = y0 + (wave & 1) * NDX + i, x = x0 + (lane >> 2);
            y = y < a.H ? y : a.H - 1;
            x = x < a.W ? x : a.W - 1;
            xpixq[i] = y * a.W + x;
        }
        xl_seg = 0; c_in = 0;
        seg_select();
    };
    auto issue_x = [&]() {       // the next chunk of the stream -> ring slot xl_cnt % NXR
        const float* base = sbase + c_in;
        const unsigned dst = xb_lds + (unsigned)(((xl_cnt % NXR) * XSLOT + (wave & 1) * NDX * 256) * 4);
#pragma unroll
        for (int i = 0; i < NDX; ++i) dma16(base, xvoff[i], dst + i * 1024);
        ++xl_cnt;
        c_in += CK;
        if (c_in >= C) {
            c_in = 0;
            if (++xl_seg == NSEG) {
                xl_unit += t_stride;
                if (xl_unit < t_hi) { xl_it = decode(xl_unit); xl_setup(); }
            } else {
                seg_select();
            }
        }
    };
    // ---- W ring loader (waves 2-3): NS slices per unit, the same for every unit.  The paired forward's stream is the
    //      unpaired one (W_f | W_c, 3 NR slices): steps 3 NR .. 5 NR - 1 (the second half's s1 and clustering phases)
    //      read slices NR .. 3 NR - 1 again.
    int wl_step = 0, wl_cnt = 0;
    unsigned wvoff[NDW];
    bool wact[NDW];
#pragma unroll
    for (int i = 0; i < NDW; ++i) {
        const int row = ((wave & 1) * NDW + i) * 16 + (lane >> 2);
        wact[i] = ((wave & 1) * NDW + i) * 16 < C;
        wvoff[i] = (unsigned)(row * 64 + (((lane & 3) ^ swz(row)) * 16));
    }
    auto issue_w = [&]() {
        const float* p = a.w + (long long)((PAIR && wl_step >= 3 * NR) ? wl_step - 2 * NR : wl_step) * WSLOT;
        const unsigned dst = wb_lds + (unsigned)(((wl_cnt % NWR) * WSLOT + (wave & 1) * NDW * 256) * 4);
#pragma unroll
        for (int i = 0; i < NDW; ++i)
            if (wact[i]) dma16(p, wvoff[i], dst + i * 1024);
        ++wl_cnt;
        if (++wl_step == NS) wl_step = 0;
    };

    // ---- fragments: pixel row 16*wave + lp / weight row 16*t + lp; this lane's quad lg, swizzled by the row
    const int qoff = (lg ^ swz(lp)) * 4;          // (16*wave + lp) and (16*t + lp) have the same (row >> 2) & 3
    const int arow = (16 * wave + lp) * CK + qoff;
    const int brow = lp * CK + qoff;              // + 16*t rows
    f32x4 afA, afB, bfA[NT], bfB[NT];             // two fragment sets: the next step's reads fly under this step's MFMAs
    auto read_a = [&](const float* xb, f32x4& af) { af = *reinterpret_cast<const f32x4*>(xb + arow); };
    auto read_b = [&](const float* wb, f32x4 (&bf)[NT]) {
#pragma unroll
        for (int t = 0; t < NT; ++t) bf[t] = *reinterpret_cast<const f32x4*>(wb + brow + 16 * t * CK);
    };

    f32x4 Ra[NT], Rt[NT], Rz[(BWD || PAIR) ? NT : 1];
    auto init_acc = [&](f32x4 (&R)[NT], int which) {
#pragma unroll
        for (int t = 0; t < NT; ++t) R[t] = *reinterpret_cast<const f32x4*>(img + which * C + 16 * t + 4 * lg);
    };

    // ---- pipeline state
    int gs = 0;        // global step of this workgroup: its weight slice sits in ring slot gs % NWR
    int xc = 0;        // next X chunk to be consumed: ring slot xc % NXR
    // Loader part of a step (before the barrier that publishes the next stage): issue what lies D stages ahead, then
    // wait until the NEXT stage's data has landed (everything but the D - 1 younger stages).  x_step: this step consumed
    // an X chunk (the X ring advances only then).
    auto loader = [&](bool x_step) {
        if (xrole) {
            if (x_step && xl_cnt < total_xchunks) issue_x();
            if (xl_cnt - (xc + (x_step ? 1 : 0)) >= DX) dma_wait<NDX * (DX - 1)>(); else dma_wait<0>();
        } else {
            if (wl_cnt < total_steps) issue_w();
            if (wl_cnt - (gs + 1) >= DW) dma_wait<NDW * (DW - 1)>(); else dma_wait<0>();
        }
    };

    // Two steps whose pixel operand comes from LDS (chunks xc, xc + 1), fragment sets A then B.  next_lds: the step after
    // the pair also reads an X chunk.  (LDS phases always have an even number of steps: NR is even for C >= 32.)
    auto lds_pair = [&](f32x4 (&acc)[NT], bool next_lds) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4& af = h ? afB : afA;
            f32x4(&bf)[NT] = h ? bfB : bfA;
            f32x4& afn = h ? afA : afB;
            f32x4(&bfn)[NT] = h ? bfA : bfB;
            const bool has_next = gs + 1 < total_steps;
            const bool nl = h == 0 || next_lds;
            loader(true);
            ring_publish();                      // stage gs + 1 (and chunk xc + 1) is in LDS for everybody
            if (has_next) {
                read_b(Wb + ((gs + 1) % NWR) * WSLOT, bfn);
                if (nl) read_a(Xb + ((xc + 1) % NXR) * XSLOT, afn);
            }
            // tile pairs outermost: a pair's two chains alternate (dependent MFMAs 64 cycles apart, latency 40) and its
            // weight fragments die after 8 MFMAs, so the registers of set A and of the incoming set B overlap
#pragma unroll
            for (int t = 0; t < NT; t += 2)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[t] = mfma16(bf[t][j], af[j], acc[t]);
                    acc[t + 1] = mfma16(bf[t + 1][j], af[j], acc[t + 1]);
                }
            ++gs; ++xc;
        }
    };
    // NR steps whose pixel operand is the register tile `op` (a previous result); next_lds refers to the step after the
    // last one (the first step of the next LDS phase consumes chunk xc).
    auto reg_steps = [&](const f32x4 (&op)[NT], f32x4 (&acc)[NT], bool next_lds) {
#pragma unroll
        for (int c = 0; c < NR; ++c) {
            f32x4(&bf)[NT] = (c & 1) ? bfB : bfA;
            f32x4(&bfn)[NT] = (c & 1) ? bfA : bfB;
            f32x4& afn = (c & 1) ? afA : afB;
            const bool has_next = gs + 1 < total_steps;
            const bool nl = (c == NR - 1) && next_lds;
            loader(false);
            ring_publish();
            if (has_next) {
                read_b(Wb + ((gs + 1) % NWR) * WSLOT, bfn);
                if (nl) read_a(Xb + (xc % NXR) * XSLOT, afn);
            }
#pragma unroll
            for (int t = 0; t < NT; t += 2)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[t] = mfma16(bf[t][j], op[c][j], acc[t]);
                    acc[t + 1] = mfma16(bf[t + 1][j], op[c][j], acc[t + 1]);
                }
            ++gs;
        }
    };

    // ---- per-lane output geometry of the current unit: pixel (row wave, column lp) of the tile, channels 16 t + 4 lg ..
    UnitIt ep_it = decode(t_first);
    int ep_unit = t_first;
    bool pok = false;
    int pix = 0;
    long long row0 = 0;           // wave-uniform: the first pixel of the wave's tile row
    auto ep_setup = [&]() {
        const int y = ep_it.ty * TH + wave, x0 = ep_it.tx * TW, x = x0 + lp;
        pok = y < a.H && x < a.W;
        pix = y * a.W + x;
        row0 = (long long)y * a.W + x0;
    };
    const long long img_elems = (long long)a.H * a.W;
    // A store's address = wave-uniform 64-bit part (plane, tile row; pinned to scalar registers, or the compiler folds the
    // lane offset into the loop-invariant plane pointer instead) + this lane's constant 32-bit offset: one register for the
    // whole kernel where per-lane 64-bit pointers to each output were kept alive across the unit loop.
    const unsigned lane_off = (unsigned)(lp * C + 4 * lg);
    auto uniform = [](float* p) {
        const unsigned long long v = reinterpret_cast<unsigned long long>(p);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        return reinterpret_cast<float*>(((unsigned long long)hi << 32) | lo);
    };
    auto store_tile = [&](const f32x4 (&R)[NT], float* base) {     // base: batch plane [H][W][C]
        if (!pok) return;
        float* p = uniform(base + row0 * C) + lane_off;
#pragma unroll
        for (int t = 0; t < NT; ++t) stg16(p + 16 * t, R[t]);
    };
    auto wsum = [&](float v) {      // over the four lanes (channel quads) that share a pixel
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        return v;
    };

    // ---- forward: LayerNorm over the C channels of each pixel of z in Ra (4 NT registers in each of the pixel's four
    //      lanes); stores yhat and rstd at batch bb and leaves y = yhat*gamma + beta in Ra
    auto layer_norm = [&](int bb) {
        float rstd;
        {
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) s += (Ra[t][0] + Ra[t][1]) + (Ra[t][2] + Ra[t][3]);
            const float mu = wsum(s) * (1.f / C);
            float q = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = Ra[t][k] - mu;
                    Ra[t][k] = d;
                    q += d * d;
                }
            rstd = 1.f / sqrtf(wsum(q) * (1.f / C) + a.eps);
#pragma unroll
            for (int t = 0; t < NT; ++t) Ra[t] *= rstd;
        }
        store_tile(Ra, a.out0 + (long long)bb * img_elems * C);
        if (pok && lg == 0) a.out2[(long long)bb * img_elems + pix] = rstd;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const f32x4 gq = *reinterpret_cast<const f32x4*>(img + 2 * C + 16 * t + 4 * lg);
            const f32x4 bq = *reinterpret_cast<const f32x4*>(img + 3 * C + 16 * t + 4 * lg);
            Ra[t] = Ra[t] * gq + bq;
        }
    };

    // ---- prologue: fill the rings DX / DW stages deep, publish stage 0
    if (xrole) {
        xl_setup();
        for (int k = 0; k < DX && xl_cnt < total_xchunks; ++k) issue_x();
    } else {
        for (int k = 0; k < DW && wl_cnt < total_steps; ++k) issue_w();
    }
    dma_wait<0>();
    ring_publish();
    read_a(Xb, afA);
    read_b(Wb, bfA);
    init_acc(Ra, BWD ? 4 : 0);
    // Steps alternate between the fragment sets A and B; every phase has an even number of steps, so each phase starts on A.
    static_assert(NR % 2 == 0, "C must be a multiple of 32");

    for (; ep_unit < t_hi; ep_unit += t_stride) {
        ep_it = decode(ep_unit);
        ep_setup();
        const bool more_units = ep_unit + t_stride < t_hi;
        if constexpr (!BWD) {
            if constexpr (!PAIR) {
                // ---- z = convf(cat[s0, s1]) + b_f
                for (int i = 0; i < NXC; i += 2) lds_pair(Ra, i + 2 < NXC);
                layer_norm(ep_it.b);
                // ---- centre = clustering(y) + b_c, pixel operand = the registers of y
                init_acc(Rt, 1);
                reg_steps(Ra, Rt, more_units);
                store_tile(Rt, a.out1 + (long long)ep_it.b * img_elems * C);
            } else {
                // ---- the shared half of z: b_f + W_f[:, :C] s0, kept in Rz for the second batch
                for (int i = 0; i < NR; i += 2) lds_pair(Ra, true);
#pragma unroll
                for (int t = 0; t < NT; ++t) Rz[t] = Ra[t];
                // ---- batch b, then batch b + n: + W_f[:, C:] s1, LayerNorm, clustering
                for (int half = 0; half < 2; ++half) {
                    const int bb = ep_it.b + half * a.n;
                    for (int i = 0; i < NR; i += 2) lds_pair(Ra, i + 2 < NR);
                    layer_norm(bb);
                    init_acc(Rt, 1);
                    reg_steps(Ra, Rt, half == 0 || more_units);
                    store_tile(Rt, a.out1 + (long long)bb * img_elems * C);
                    if (half == 0) {
#pragma unroll
                        for (int t = 0; t < NT; ++t) Ra[t] = Rz[t];
                    }
                }
            }
            init_acc(Ra, 0);
        } else {
            // dz of BOTH halves stays in registers (Rz: batch b, Ra: batch b + n): the shared stream's gradient needs
            // W_f[:, :C]^T (dz[b] + dz[b + n]) -- ONE register-operand GEMM on the sum instead of two (5 C^2 instead of
            // 6 C^2 multiply-adds per pixel pair half), and d s0 is written once.
            for (int half = 0; half < 2; ++half) {
                const int bb = ep_it.b + half * a.n;
                // ---- dy = W_c^T dcentre
                for (int i = 0; i < NR; i += 2) lds_pair(Ra, half == 0 || i + 2 < NR);
                // ---- LayerNorm backward: g = dy*gamma, dz = rstd * (g - yhat*mean(g*yhat) - mean(g))
                const float* const yh = a.in0 + (long long)bb * img_elems * C + (long long)pix * C + 4 * lg;
                const float rstd = pok ? a.in1[(long long)bb * img_elems + pix] : 0.f;
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const f32x4 gq = *reinterpret_cast<const f32x4*>(img + 2 * C + 16 * t + 4 * lg);
                    const f32x4 yq = ldg16(pok ? yh + 16 * t : g_zero4c);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float g = Ra[t][k] * gq[k];
                        Ra[t][k] = g;
                        s1 += g;
                        s2 += g * yq[k];
                    }
                }
                const float m1 = wsum(s1) * (1.f / C), m2 = wsum(s2) * (1.f / C);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const f32x4 yq = ldg16(pok ? yh + 16 * t : g_zero4c);
#pragma unroll
                    for (int k = 0; k < 4; ++k) Ra[t][k] = rstd * (Ra[t][k] - yq[k] * m2 - m1);
                }
                store_tile(Ra, a.out0 + (long long)bb * img_elems * C);
                if (half == 0) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) Rz[t] = Ra[t];
                    init_acc(Ra, 4);
                }
            }
            // ---- d s1, written for the batch the forward READ s1 from: batch b's dz goes to b + n and vice versa
            init_acc(Rt, 4);
            reg_steps(Rz, Rt, false);                                          // W_f[:, C:]^T dz[b]
            store_tile(Rt, a.out1 + (long long)(ep_it.b + a.n) * img_elems * C);
            init_acc(Rt, 4);
            reg_steps(Ra, Rt, false);                                          // W_f[:, C:]^T dz[b + n]
            store_tile(Rt, a.out1 + (long long)ep_it.b * img_elems * C);
            // ---- d s0 = add + W_f[:, :C]^T (dz[b] + dz[b + n])
#pragma unroll
            for (int t = 0; t < NT; ++t) Rz[t] += Ra[t];
            init_acc(Rt, 4);
            if (a.res.ptr && pok) {
                const float* rp = src_batch_ptr(a.res, ep_it.b) + (long long)pix * a.res.pix_stride + 4 * lg;
#pragma unroll
                for (int t = 0; t < NT; ++t) Rt[t] = ldg16(rp + 16 * t);
            }
            reg_steps(Rz, Rt, more_units);
            store_tile(Rt, a.out2 + (long long)ep_it.b * img_elems * C);
            init_acc(Ra, 4);
        }
    }
}

// LayerNorm affine gradients from the pixel-reduction GEMM of the clustering convolution taken on yhat:
//   G[co][ci] = sum_px dcentre[px][co] yhat[px][ci],   dbc[co] = sum_px dcentre[px][co]
//   dW_c[co][ci] = gamma[ci] G[co][ci] + dbc[co] beta[ci]        (y = yhat*gamma + beta)
//   dgamma[ci]   = sum_co W_c[co][ci] G[co][ci]                    (= sum_px dy*yhat, dy = W_c^T dcentre)
//   dbeta[ci]    = sum_co W_c[co][ci] dbc[co]                      (= sum_px dy)
// Block = 32 columns ci x 32 row groups (co = part, part + 32, ...: four dependent global round trips per thread, the
// kernel is pure latency): partial column sums meet in LDS.  Results are written
// (accumulate = 0) or added (1) to dwc / dgamma / dbeta (dwc may be G itself); dbc_out, if given, receives dbc the same
// way (the clustering bias gradient on its way to its accumulator).
__global__ __launch_bounds__(1024) void affine_grads_kernel(const float* G, const float* __restrict__ dbc, const float* __restrict__ Wc,
                                    const float* __restrict__ gamma, const float* __restrict__ beta, int C, float* dwc,
                                    float* __restrict__ dbc_out, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                    int accumulate) {
    constexpr int NPART = 32;
    __shared__ float red[2][NPART][32];
    const int cl = threadIdx.x & 31, part = threadIdx.x >> 5, ci = blockIdx.x * 32 + cl;
    float dg = 0.f, db = 0.f;
    if (ci < C) {
        const float gm = gamma[ci], bt = beta[ci];
        for (int co = part; co < C; co += NPART) {
            const float g = G[co * C + ci], w = Wc[co * C + ci], d = dbc[co];
            dg += w * g;
            db += w * d;
            const float v = gm * g + d * bt;
            dwc[co * C + ci] = accumulate ? dwc[co * C + ci] + v : v;
        }
    }
    red[0][part][cl] = dg;
    red[1][part][cl] = db;
    __syncthreads();
    if (part == 0 && ci < C) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int k = 0; k < NPART; ++k) { a += red[0][k][cl]; b += red[1][k][cl]; }
        dgamma[ci] = accumulate ? dgamma[ci] + a : a;
        dbeta[ci] = accumulate ? dbeta[ci] + b : b;
        if (dbc_out) dbc_out[ci] = accumulate ? dbc_out[ci] + dbc[ci] : dbc[ci];
    }
}

int launch(const ChainK& k, int C, bool bwd, bool pair, hipStream_t st) {
    const int cus = bmc_num_cus();
    const int max_blocks = 2 * cus;      // resident workgroups per CU (LDS rings: ~75 KB per workgroup at C = 128)
    dim3 grid((unsigned)(k.nunits < max_blocks ? k.nunits : max_blocks)), block(256);
#define BMC_LAUNCH_CHAIN(NU_)                                                                    \
    do {                                                                                          \
        if (bwd) hipLaunchKernelGGL((chain_kernel<NU_, true>), grid, block, 0, st, k);            \
        else if (pair) hipLaunchKernelGGL((chain_kernel<NU_, false, true>), grid, block, 0, st, k); \
        else hipLaunchKernelGGL((chain_kernel<NU_, false>), grid, block, 0, st, k);               \
    } while (0)
    if (C == 128) BMC_LAUNCH_CHAIN(8);
    else if (C == 64) BMC_LAUNCH_CHAIN(4);
    else BMC_LAUNCH_CHAIN(2);
#undef BMC_LAUNCH_CHAIN
    return 0;
}

bool src_ok(const bmc_src_t& s, int C) {
    return s.ptr && s.nch == C && s.pix_stride % 4 == 0 && s.batch_stride % 4 == 0 && ((uintptr_t)s.ptr & 15) == 0;
}

// Host image of src_batch_ptr: the element offset of launch batch b.
long long src_batch_off(const bmc_src_t& s, int b) {
    long long bs = (long long)b + s.batch_shift;
    if (s.batch_mod > 0) bs %= s.batch_mod;
    return bs * s.batch_stride;
}

// The forward launch can walk pairs (b, b + B/2) when s0 gives both batches of every pair the same image.
// -> nullptr, or the reason why not.
const char* fwd_unpairable(const bmc_chain_fwd_args_t& h) {
    if (h.B % 2) return "B is odd";
    if (h.s0.batch_mod == BMC_SRC_TABLE) return "s0 is a pointer table";
    const int n = h.B / 2;
    for (int b = 0; b < n; ++b)
        if (src_batch_off(h.s0, b) != src_batch_off(h.s0, b + n)) return "s0 maps batches b and b + B/2 to different images";
    return nullptr;
}

// Pair when the fullest CU then runs fewer steps.  A pair costs 5 NR steps where a unit costs 3 NR, and the two workgroups
// resident on a CU share its matrix pipes, so the launch takes as long as the CU with the most steps: 5 ceil(P / CUs)
// against 3 ceil(2P / CUs) for P pairs.  (Counting rounds of the 2 x CUs workgroups instead mispredicted three of ten
// measured shapes: NOTEBOOK R11.)  Up to one pair per CU the launch stays unpaired: a single workgroup on a CU cannot hide
// its own LayerNorm and barrier phases, and two 3 NR units beside each other measured faster than one 5 NR pair.
bool fwd_pair_rule(long long pairs, int cus) {
    return pairs > cus && 5 * ((pairs + cus - 1) / cus) < 3 * ((2 * pairs + cus - 1) / cus);
}

}  // namespace

extern "C" int bmc_chain_fwd(const bmc_chain_fwd_args_t* h, bmc_stream_t stream) {
    BMC_CHECK_ARG(h != nullptr, "bmc_chain_fwd: null args");
    BMC_CHECK_ARG(h->C == 32 || h->C == 64 || h->C == 128, "bmc_chain_fwd: C=%d unsupported (32, 64, 128)", h->C);
    BMC_CHECK_ARG(h->B > 0 && h->H > 0 && h->W > 0, "bmc_chain_fwd: bad shape");
    BMC_CHECK_ARG(src_ok(h->s0, h->C) && src_ok(h->s1, h->C), "bmc_chain_fwd: sources must carry C channels, 16-byte aligned");
    BMC_CHECK_ARG(h->wstream && h->bias_f && h->bias_c && h->gamma && h->beta && h->yhat && h->rstd && h->centre,
                  "bmc_chain_fwd: null pointer");
    ChainK k = {};
    k.src[0] = to_dev(h->s0); k.src[1] = to_dev(h->s1);
    k.w = h->wstream;
    k.vec[0] = h->bias_f; k.vec[1] = h->bias_c; k.vec[2] = h->gamma; k.vec[3] = h->beta;
    k.eps = h->eps;
    k.out0 = h->yhat; k.out1 = h->centre; k.out2 = h->rstd;
    k.nb = h->B; k.n = 0; k.H = h->H; k.W = h->W;
    k.tiles_x = (h->W + TW - 1) / TW; k.tiles_y = (h->H + TH - 1) / TH;
    long long nu = (long long)h->B * k.tiles_x * k.tiles_y;
    BMC_CHECK_ARG(nu < (1ll << 31), "bmc_chain_fwd: too many tiles");
    // BMC_CHAIN_PAIR (tests and experiments, read per launch): 0 = never pair, 1 = pair or refuse, unset = the rule
    const char* const e = getenv("BMC_CHAIN_PAIR");
    const int mode = e ? atoi(e) : -1;
    bool pair = false;
    if (mode != 0) {
        const char* const why = fwd_unpairable(*h);
        BMC_CHECK_ARG(mode != 1 || !why, "bmc_chain_fwd: BMC_CHAIN_PAIR=1 but the launch cannot be paired: %s", why);
        pair = !why && (mode == 1 || fwd_pair_rule(nu / 2, bmc_num_cus()));
    }
    if (pair) {
        nu /= 2;
        k.nb = h->B / 2; k.n = h->B / 2;
    }
    k.nunits = (int)nu;
    launch(k, h->C, false, pair, (hipStream_t)stream);
    BMC_CHECK_LAUNCH("bmc_chain_fwd");
    return 0;
}

extern "C" int bmc_chain_bwd(const bmc_chain_bwd_args_t* h, bmc_stream_t stream) {
    BMC_CHECK_ARG(h != nullptr, "bmc_chain_bwd: null args");
    BMC_CHECK_ARG(h->C == 32 || h->C == 64 || h->C == 128, "bmc_chain_bwd: C=%d unsupported (32, 64, 128)", h->C);
    BMC_CHECK_ARG(h->n > 0 && h->H > 0 && h->W > 0, "bmc_chain_bwd: bad shape");
    BMC_CHECK_ARG(src_ok(h->dcentre, h->C), "bmc_chain_bwd: dcentre must carry C channels, 16-byte aligned");
    BMC_CHECK_ARG(h->wstream && h->gamma && h->yhat && h->rstd && h->dz && h->ds1 && h->ds0, "bmc_chain_bwd: null pointer");
    BMC_CHECK_ARG(!h->ds0_add.ptr || (h->ds0_add.pix_stride % 4 == 0 && ((uintptr_t)h->ds0_add.ptr & 15) == 0),
                  "bmc_chain_bwd: ds0_add must be 16-byte granular");
    ChainK k = {};
    k.src[0] = to_dev(h->dcentre); k.src[1] = k.src[0];
    k.w = h->wstream;
    k.vec[2] = h->gamma;
    k.out0 = h->dz; k.out1 = h->ds1; k.out2 = h->ds0;
    k.in0 = h->yhat; k.in1 = h->rstd;
    k.res = to_dev(h->ds0_add);
    k.nb = h->n; k.n = h->n; k.H = h->H; k.W = h->W;
    k.tiles_x = (h->W + TW - 1) / TW; k.tiles_y = (h->H + TH - 1) / TH;
    const long long nu = (long long)h->n * k.tiles_x * k.tiles_y;
    BMC_CHECK_ARG(nu < (1ll << 31), "bmc_chain_bwd: too many tiles");
    k.nunits = (int)nu;
    launch(k, h->C, true, false, (hipStream_t)stream);
    BMC_CHECK_LAUNCH("bmc_chain_bwd");
    return 0;
}

extern "C" int bmc_chain_affine_grads(const float* G, const float* dbc, const float* Wc, const float* gamma, const float* beta,
                                      int C, float* dwc, float* dbc_out, float* dgamma, float* dbeta, int accumulate,
                                      bmc_stream_t stream) {
    BMC_CHECK_ARG(G && dbc && Wc && gamma && beta && dwc && dgamma && dbeta && C > 0, "bmc_chain_affine_grads: bad arguments");
    hipLaunchKernelGGL(affine_grads_kernel, dim3((C + 31) / 32), dim3(1024), 0, (hipStream_t)stream, G, dbc, Wc, gamma, beta, C, dwc, dbc_out,
                       dgamma, dbeta, accumulate);
    BMC_CHECK_LAUNCH("bmc_chain_affine_grads");
    return 0;
}
