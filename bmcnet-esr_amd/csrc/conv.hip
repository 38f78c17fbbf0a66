// Implicit-GEMM 3x3 / 1x1 convolution on the fp32 matrix cores of gfx950
// (v_mfma_f32_32x32x2_f32), NHWC, multi-source (no torch.cat), fused
// bias / residual / ReLU / ReLU-mask epilogue, optional per-group weights.
//
// One workgroup (4 waves) computes an 8x16-pixel x BN-channel output tile.
// K = taps * sum(nch) is walked in steps of (one 16-channel chunk, one tap):
//   * the (8+2)x(16+2) input halo of the chunk is staged once in LDS and re-read
//     for all 9 taps (tap shift = constant LDS offset);
//   * the [BN][16] weight slice of the step is streamed through a second LDS
//     buffer; both are double-buffered, global loads for step s+1 are issued
//     before the MFMAs of step s and written to LDS after them (one barrier/step).
// MFMA operand mapping: A = pixels (rows), B = output channels (cols); lane
// (i = l&31, h = l>>5) reads 4 consecutive k at offset 4h with one ds_read_b128 --
// the k-order inside a chunk is permuted identically for A and B, which a dot
// product does not care about.
#include "bmc_common.h"
#include "conv_k.h"
#include "dma_ring.h"
#include "tile_walk.h"
#include <stdlib.h>

namespace {

constexpr int CK = BMC_CK;  // channels per chunk
constexpr int RS = 20;      // LDS row stride in floats (16 + 4 pad: conflict-free ds_read_b128)
constexpr int TW = 16;      // tile width; the tile height TH (8 or 4 rows) is a kernel template parameter

// Tile shapes (4 waves): BN = 128: waves 2(px) x 2(ch), wave = (TH/2 rows x 16) px x 64 ch  [TH = 8: 2x2 MFMA tiles, TH = 4: 1x2]
//                        BN =  64: waves 2 x 2,           wave = (TH/2 rows x 16) px x 32 ch  [small problems: 4x the workgroups]
//                        BN =  32: waves 4(px) x 1,       wave = 32 px x 32 ch (TH = 8)        [narrow outputs]
template <int TAPS, int BN, int TH>
__global__ __launch_bounds__(256, (BN == 128 && TH == 8) ? 3 : 4) void conv_kernel(const ConvK a) {
    static_assert((BN == 32 && TH == 8) || ((BN == 128 || BN == 64) && (TH == 8 || TH == 4)), "unsupported tile shape");
    constexpr int P = TAPS == 9 ? 1 : 0;
    constexpr int HWD = TW + 2 * P, HHT = TH + 2 * P, NHALO = HWD * HHT;
    constexpr int MT = BN == 32 ? 1 : TH / 4, NT = BN == 128 ? 2 : 1;
    constexpr int NXLD = (NHALO * 4 + 255) / 256;
    constexpr int NWLD = (BN * 4 + 255) / 256;
    // Halo rows start on a 64-float (256-byte = all 64 banks) boundary: ds_read_b128 is served in the 16-lane groups
    // {0-3,12-15,20-27} / {4-11,16-19,28-31} (MI355X_MICROARCH.md, LDS), i.e. 8 pixels of one halo row and 8 of the next.
    // With 20-float pixels a pixel's bank quad is 5 hx (mod 16): the two half-groups of one row are disjoint sets of quads,
    // and stay disjoint across the two rows exactly when the row stride is a multiple of 16 quads -- 18 x 20 = 360 floats
    // was not (PMC: 40 % of the LDS cycles of the round-2 kernel were bank conflicts), 384 is (1x1: 16 x 20 = 320 already).
    constexpr int XROW = (HWD * RS + 63) / 64 * 64;
    constexpr int XBUF = HHT * XROW, WBUF = BN * RS;
    __shared__ __attribute__((aligned(16))) float lds[2 * XBUF + 2 * WBUF + BMC_MAX_SRC * 8 + BN];
    float* const Xb = lds;
    float* const Wb = lds + 2 * XBUF;
    SrcDev* const tab = reinterpret_cast<SrcDev*>(lds + 2 * XBUF + 2 * WBUF);   // source table (runtime-indexed)
    float* const init_lds = lds + 2 * XBUF + 2 * WBUF + BMC_MAX_SRC * 8;     // accumulator start values (bias or zeros: bias_start_values, conv_k.h)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const bool bias_pre = a.bias != nullptr && a.batch_per_group >= a.B && a.ntn == 1;
    BMC_LOAD_SRC_TABLE(tab, a, tid);
    if (tid < BN) init_lds[tid] = (bias_pre && tid < a.Cout) ? a.bias[tid] : 0.f;
    __syncthreads();
    // tile_walk() of tile_walk.h, written out, like bias_start_values() (conv_k.h) above: with the calls this kernel's
    // scalar registers are allocated differently (up to 5 more of them spilled, other v_readlane / v_writelane counts),
    // with the same code in place they are not.
    const int ntiles = a.ntiles;
    const bool xcd_map = (gridDim.x % NUM_XCD) == 0 && ntiles >= (int)gridDim.x;
    const int xcd = blockIdx.x % NUM_XCD, xj = blockIdx.x / NUM_XCD, per_x = gridDim.x / NUM_XCD;
    const int t_lo = xcd_map ? (int)((long long)ntiles * xcd / NUM_XCD) : 0;
    const int t_hi = xcd_map ? (int)((long long)ntiles * (xcd + 1) / NUM_XCD) : ntiles;
    const int t_first = xcd_map ? t_lo + xj : (int)blockIdx.x;
    const int t_stride = xcd_map ? per_x : (int)gridDim.x;
    const int my_tiles = t_first < t_hi ? (t_hi - t_first + t_stride - 1) / t_stride : 0;
    const int nsteps = a.nchunks * TAPS;
    const int total_steps = my_tiles * nsteps, total_chunks = my_tiles * a.nchunks;
    if (my_tiles == 0) return;   // block-uniform
    const long long wstep = (long long)a.Coutpad * CK;

    // the three users of a tile's coordinates (X loader, W loader, epilogue) each walk their own copy of the digits
    using TileIt = Tile3;
    const TileIt it0 = tile_decode(t_first, a.ntn, a.tiles_x, a.tiles_y), stp = tile_decode(t_stride, a.ntn, a.tiles_x, a.tiles_y);
    auto it_next = [&](TileIt& it) { it = tile_advance(it, stp, a.ntn, a.tiles_x, a.tiles_y); };
    TileIt xl_it = it0, wl_it = it0, ep_it = it0;
    const int q4 = (tid & 3) * 4;

    // ---- X loader: walks (tile, chunk) in consumption order
    int xl_tile = t_first, xl_chunk = 0, xl_b = 0, s_idx = 0, c_in = 0;
    const float* sbase = nullptr;   // current source: batch base pointer, pixel stride, channel count
    int spix = 0, snch = 0;
    auto src_select = [&]() {
        const SrcDev S = tab[s_idx];
        sbase = src_batch_ptr(S, xl_b); spix = S.pix_stride; snch = S.nch;
    };
    int xpix[NXLD];
    bool xok[NXLD];
    auto xl_setup = [&]() {      // for the tile xl_it points at
        const int y0 = xl_it.ty * TH, x0 = xl_it.tx * TW;
        xl_b = xl_it.b;
#pragma unroll
        for (int n = 0; n < NXLD; ++n) {
            const int e = tid + 256 * n, hp = e >> 2;
            const int hy = hp / HWD, hx = hp - hy * HWD;
            const int y = y0 - P + hy, x = x0 - P + hx;
            xok[n] = hp < NHALO && y >= 0 && y < a.H && x >= 0 && x < a.W;   // out-of-image lanes read a zero buffer: no
            xpix[n] = y * a.W + x;                                           // branch, and nothing to fix up after the load
        }
        s_idx = 0; c_in = 0; xl_chunk = 0;
        src_select();
    };
    // X register ring depth = how many steps a 1x1 tile load runs ahead (deeper rings, 2 and 3, measured no gain: the 1x1
    // kernel is power / clock limited)
    constexpr int LX = 1;
    f32x4 xr[LX][NXLD], wr[NWLD];
    int xlds[NXLD];              // LDS offset of this thread's halo piece (tile-independent)
#pragma unroll
    for (int n = 0; n < NXLD; ++n) {
        const int hp = (tid + 256 * n) >> 2, hy = hp / HWD;
        xlds[n] = hy * XROW + (hp - hy * HWD) * RS + q4;
    }
    auto load_x = [&](int slot) {
        const float* base = sbase + c_in + q4;
#pragma unroll
        for (int n = 0; n < NXLD; ++n) xr[slot][n] = ldg16(xok[n] ? base + (long long)xpix[n] * spix : g_zero4);
        c_in += CK;
        if (++xl_chunk == a.nchunks) {
            xl_tile += t_stride;
            if (xl_tile < t_hi) { it_next(xl_it); xl_setup(); }
        } else if (c_in >= snch) {
            c_in = 0; ++s_idx;
            src_select();
        }
    };
    auto store_x = [&](int slot, int buf) {
#pragma unroll
        for (int n = 0; n < NXLD; ++n) {
            const int e = tid + 256 * n, hp = e >> 2;
            if (hp < NHALO) *reinterpret_cast<f32x4*>(Xb + buf * XBUF + xlds[n]) = xr[slot][n];
        }
    };
    // ---- W loader: walks (tile, step)
    int wl_tile = t_first, wl_step = 0;
    const float* wl_base = nullptr;
    auto wl_setup = [&]() {      // for the tile wl_it points at
        const int grp = a.batch_per_group >= a.B ? 0 : wl_it.b / a.batch_per_group;
        wl_base = static_cast<const float*>(a.w) + (long long)grp * a.w_group_stride + (long long)wl_it.nt * BN * CK;
        wl_step = 0;
    };
    auto load_w = [&]() {
        const float* p = wl_base + (long long)wl_step * wstep;
#pragma unroll
        for (int n = 0; n < NWLD; ++n) {
            const int e = tid + 256 * n;
            // no branch around the load (a divergent branch makes the compiler serialise the loads with vmcnt(0)):
            // lanes past the slice re-read its last piece and never store it
            const int ec = (n + 1) * 256 <= BN * 4 ? e : (e < BN * 4 ? e : BN * 4 - 1);
            wr[n] = ldg16(p + ec * 4);
        }
        if (++wl_step == nsteps) {
            wl_tile += t_stride;
            if (wl_tile < t_hi) { it_next(wl_it); wl_setup(); }
        }
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int n = 0; n < NWLD; ++n) {
            const int e = tid + 256 * n;
            if ((n + 1) * 256 <= BN * 4 || e < BN * 4) *reinterpret_cast<f32x4*>(Wb + buf * WBUF + (e >> 2) * RS + q4) = wr[n];
        }
    };

    // ---- MFMA fragment addressing
    const int rowbase = BN == 32 ? 2 * wave : (TH / 2) * (wave >> 1);
    const int cobase = BN == 32 ? 0 : (BN / 2) * (wave & 1);
    int aoff[MT], boff[NT];
#pragma unroll
    for (int t = 0; t < MT; ++t) aoff[t] = (rowbase + 2 * t + (li >> 4)) * XROW + (li & 15) * RS + 4 * lh;
#pragma unroll
    for (int u = 0; u < NT; ++u) boff[u] = (cobase + 32 * u + li) * RS + 4 * lh;

    f32x16 acc[MT][NT];
    auto init_acc = [&]() {     // see init_lds above
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(init_lds + cobase + 4 * lh + 32 * u + 8 * rq);
#pragma unroll
                for (int t = 0; t < MT; ++t)
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[t][u][4 * rq + k] = v[k];
            }
    };
    init_acc();

    // Software pipeline (one barrier per step, MFMA work queued on both sides of it):
    //   top of step s : read fragments (s, k-half 1); write W(s+1) [and the next chunk's X on a chunk's last tap] to
    //                   LDS from registers loaded one step earlier; 16 MFMAs on fragments (s, k-half 0)
    //   barrier
    //   after barrier : read fragments (s+1, k-half 0); issue global loads for W(s+2) [/ next X];
    //                   16 MFMAs on fragments (s, k-half 1) -- they cover the LDS latency of the reads just issued
    f32x4 af0[MT], bf0[NT], af1[MT], bf1[NT];
    auto read_frags = [&](const float* xb, const float* wb, int tapoff, int kg, f32x4 (&af)[MT], f32x4 (&bf)[NT]) {
#pragma unroll
        for (int t = 0; t < MT; ++t) af[t] = *reinterpret_cast<const f32x4*>(xb + aoff[t] + tapoff + 8 * kg);
#pragma unroll
        for (int u = 0; u < NT; ++u) bf[u] = *reinterpret_cast<const f32x4*>(wb + boff[u] + 8 * kg);
    };
    auto mfma16 = [&](const f32x4 (&af)[MT], const f32x4 (&bf)[NT]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int u = 0; u < NT; ++u)
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[u][j], af[t][j], acc[t][u], 0, 0, 0);
    };
    auto tap_off = [](int tap) { return TAPS == 9 ? (tap / 3) * XROW + (tap % 3) * RS : 0; };

    // Epilogue: bias / residual / ReLU / mask / accumulate, 16-byte accesses, then clear the accumulators.
    // MFMA rows = output channels (registers), cols = pixels (lanes): each lane owns, for ITS pixel, four consecutive
    // channels per register quad.  ALL loads of the epilogue come before ALL its stores: vmcnt completes in order and
    // counts stores, so a load issued after a store waits for that store's round trip to HBM -- the former
    // (load, wait, store) per quad serialised 16 store round trips per tile.  Pass 1 finishes the values in place, one
    // 32x32 MFMA tile (4 quads = 4 independent loads per operand) at a time; pass 2 is nothing but stores.
    auto epilogue = [&](int) {    // for the tile ep_it points at; advances it
        const int b = ep_it.b, y0 = ep_it.ty * TH, x0 = ep_it.tx * TW, nt = ep_it.nt;
        it_next(ep_it);
        const int g = a.batch_per_group >= a.B ? 0 : b / a.batch_per_group;
        const float* const biasg = a.bias ? a.bias + (long long)g * a.bias_group_stride : nullptr;
        float* const outb = a.out + (long long)b * a.out_batch_stride;
        const float* const resb = a.residual.ptr ? src_batch_ptr(a.residual, b) : nullptr;
        const float* const maskb = a.mask.ptr ? src_batch_ptr(a.mask, b) : nullptr;
        const int co0 = nt * BN + cobase + 4 * lh;       // + 32 u + 8 rq
        bool pok[MT];
        int pix[MT];      // pixel index inside one image: 32-bit offsets from the (uniform) per-image base pointers
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int y = y0 + rowbase + 2 * t + (li >> 4), x = x0 + (li & 15);
            pok[t] = y < a.H && x < a.W;
            pix[t] = y * a.W + x;
        }
        // the usual case -- bias already in the accumulators, nothing to read back -- is one pass: ReLU on the way out
        const bool simple = !resb && !maskb && !a.accumulate && (bias_pre || !biasg);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            if (simple) break;
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                f32x4 v[4];
                bool ok[4];
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    ok[rq] = pok[t] && co0 + 32 * u + 8 * rq < a.Cout;     // Cout is a multiple of 4: a quad is all-in or all-out
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[rq][k] = acc[t][u][4 * rq + k];
                }
                auto fetch = [&](const float* base, int off, f32x4 (&d)[4], float fill) {
#pragma unroll
                    for (int rq = 0; rq < 4; ++rq) {
                        d[rq] = f32x4{fill, fill, fill, fill};
                        if (ok[rq]) d[rq] = ldg16(base + off + co0 + 32 * u + 8 * rq);
                    }
                };
                if (biasg && !bias_pre) {     // (otherwise the accumulators started from the bias)
                    f32x4 d[4];
                    fetch(biasg, 0, d, 0.f);
#pragma unroll
                    for (int rq = 0; rq < 4; ++rq) v[rq] += d[rq];
                }
                if (resb) {
                    f32x4 d[4];
                    fetch(resb, pix[t] * a.residual.pix_stride, d, 0.f);
#pragma unroll
                    for (int rq = 0; rq < 4; ++rq) v[rq] += d[rq];
                }
                if (a.relu) {
#pragma unroll
                    for (int rq = 0; rq < 4; ++rq)
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[rq][k] = fmaxf(v[rq][k], 0.f);
                }
                if (maskb) {
                    f32x4 d[4];
                    fetch(maskb, pix[t] * a.mask.pix_stride, d, 1.f);
#pragma unroll
                    for (int rq = 0; rq < 4; ++rq)
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[rq][k] = d[rq][k] > 0.f ? v[rq][k] : 0.f;
                }
                if (a.accumulate) {
                    f32x4 d[4];
                    fetch(outb, pix[t] * a.out_pix_stride, d, 0.f);
#pragma unroll
                    for (int rq = 0; rq < 4; ++rq) v[rq] += d[rq];
                }
#pragma unroll
                for (int rq = 0; rq < 4; ++rq)
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[t][u][4 * rq + k] = v[rq][k];
            }
        }
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int u = 0; u < NT; ++u)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const int co = co0 + 32 * u + 8 * rq;
                    if (pok[t] && co < a.Cout) {
                        f32x4 v;
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] = acc[t][u][4 * rq + k];
                        if (simple && a.relu) {
#pragma unroll
                            for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
                        }
                        *reinterpret_cast<f32x4*>(outb + pix[t] * a.out_pix_stride + co) = v;
                    }
                }
        init_acc();
    };

    xl_setup();
    wl_setup();
    load_x(0);
    load_w();
    store_x(0, 0);
    store_w(0);
    if (total_steps > 1) load_w();
    if (TAPS == 1) {
#pragma unroll
        for (int j = 1; j <= LX; ++j)
            if (j < total_steps) load_x(j % LX);
    }
    __syncthreads();
    read_frags(Xb, Wb, 0, 0, af0, bf0);

    if constexpr (TAPS == 1) {
        // one step per 16-channel chunk; X tiles come from HBM, so their loads run LX steps ahead (register ring)
        int tile = t_first, cc = 0;
        for (int base = 0; base < total_steps; base += LX) {
#pragma unroll
            for (int d = 0; d < LX; ++d) {
                const int s = base + d;
                if (s < total_steps) {
                    const bool has_next = s + 1 < total_steps;
                    read_frags(Xb + (s & 1) * XBUF, Wb + (s & 1) * WBUF, 0, 1, af1, bf1);
                    if (has_next) {
                        store_w((s + 1) & 1);
                        store_x((d + 1) % LX, (s + 1) & 1);
                    }
                    mfma16(af0, bf0);
                    __syncthreads();
                    if (has_next) read_frags(Xb + ((s + 1) & 1) * XBUF, Wb + ((s + 1) & 1) * WBUF, 0, 0, af0, bf0);
                    if (s + 2 < total_steps) load_w();
                    if (s + 1 + LX < total_steps) load_x((d + 1) % LX);
                    mfma16(af1, bf1);
                    if (++cc == a.nchunks) {
                        epilogue(tile);
                        tile += t_stride;
                        cc = 0;
                    }
                }
            }
        }
    } else {
        int gs = 0, gc = 0;   // global step / chunk counters of this workgroup (LDS buffer parity)
        for (int tile = t_first; tile < t_hi; tile += t_stride) {
            for (int c = 0; c < a.nchunks; ++c, ++gc) {
                const float* const xb = Xb + (gc & 1) * XBUF;
#pragma unroll
                for (int tap = 0; tap < TAPS; ++tap, ++gs) {
                    const bool has_next = gs + 1 < total_steps;
                    const bool last_tap = tap == TAPS - 1;
                    const float* const wb = Wb + (gs & 1) * WBUF;
                    read_frags(xb, wb, tap_off(tap), 1, af1, bf1);
                    if (has_next) store_w((gs + 1) & 1);
                    // the slice after that: its loads go out as soon as the staging registers are free (a full step to land
                    // from L2; issued after the barrier they had half a step, and the store above waited for them: 4 % of the
                    // kernel by the no-weight-loads ablation)
                    if (gs + 2 < total_steps) load_w();
                    if (last_tap && gc + 1 < total_chunks) store_x(0, (gc + 1) & 1);
                    mfma16(af0, bf0);
                    __syncthreads();
                    if (has_next) {
                        const float* const xbn = last_tap ? Xb + ((gc + 1) & 1) * XBUF : xb;
                        read_frags(xbn, Wb + ((gs + 1) & 1) * WBUF, tap_off(last_tap ? 0 : tap + 1), 0, af0, bf0);
                    }
                    // the next chunk's halo tile is written to LDS at the top of this chunk's last tap: issue its
                    // global loads right at the chunk's first step (8 steps of MFMAs to land from HBM)
                    if (tap == 0 && gc + 1 < total_chunks) load_x(0);
                    mfma16(af1, bf1);
                }
            }
            // every load in flight (the next slice, issued half a step ago; the next halo, eight steps ago) lands BEFORE the
            // stores go out: vmcnt counts stores too and completes in order, so the compiler's wait in front of the next
            // step's slice store would otherwise sit out the round trip of this tile's 16 stores (-0.9 %)
            dma_wait<0>();
            epilogue(tile);
        }
    }
}

}  // namespace

extern "C" int bmc_conv(const bmc_conv_args_t* h, bmc_stream_t stream) {
    BMC_CHECK_ARG(h != nullptr, "bmc_conv: null args");
    BMC_CHECK_ARG(h->nsrc >= 1 && h->nsrc <= BMC_MAX_SRC, "bmc_conv: nsrc=%d out of range", h->nsrc);
    BMC_CHECK_ARG(h->taps == 1 || h->taps == 9, "bmc_conv: taps must be 1 or 9 (got %d)", h->taps);
    BMC_CHECK_ARG(h->B > 0 && h->H > 0 && h->W > 0, "bmc_conv: bad shape %dx%dx%d", h->B, h->H, h->W);
    BMC_CHECK_ARG(h->Cout > 0 && h->Coutpad >= h->Cout && h->Coutpad % 32 == 0 &&
                      (h->Coutpad == 32 || h->Coutpad % 128 == 0),
                  "bmc_conv: Coutpad=%d must be 32 or a multiple of 128 and >= Cout=%d", h->Coutpad, h->Cout);
    BMC_CHECK_ARG(h->wpacked && h->out, "bmc_conv: null weight/out pointer");
    BMC_CHECK_ARG(h->Cout % 4 == 0 && h->out_pix_stride % 4 == 0 && ((uintptr_t)h->out & 15) == 0 && h->out_batch_stride % 4 == 0,
                  "bmc_conv: Cout, output strides and pointer must be 16-byte granular");
    BMC_CHECK_ARG(h->batch_per_group >= 1, "bmc_conv: batch_per_group must be >= 1");
    ConvK k;
    k.nsrc = h->nsrc;
    int ktot = 0;
    for (int i = 0; i < BMC_MAX_SRC; ++i) {
        if (i < h->nsrc) {
            BMC_CHECK_ARG(h->src[i].ptr && h->src[i].nch > 0 && h->src[i].nch % CK == 0 && h->src[i].pix_stride % 4 == 0 &&
                              ((uintptr_t)h->src[i].ptr & 15) == 0 && h->src[i].batch_stride % 4 == 0,
                          "bmc_conv: source %d: nch=%d must be a multiple of 16, pointer/strides 16-byte aligned", i,
                          h->src[i].nch);
            k.src[i] = to_dev(h->src[i]);
            ktot += h->src[i].nch;
        } else {
            k.src[i] = to_dev(h->src[0]);
        }
    }
    k.w = h->wpacked; k.bias = h->bias;
    k.w_group_stride = h->w_group_stride; k.bias_group_stride = h->bias_group_stride;
    k.batch_per_group = h->batch_per_group;
    k.out = h->out; k.out_batch_stride = h->out_batch_stride; k.out_pix_stride = h->out_pix_stride;
    k.B = h->B; k.H = h->H; k.W = h->W; k.Cout = h->Cout; k.Coutpad = h->Coutpad;
    k.relu = h->relu; k.residual = to_dev(h->residual); k.mask = to_dev(h->mask); k.accumulate = h->accumulate;
    // batch segment: images b >= seg_b of an operand come from a second tensor of the same geometry (same strides: the per-image
    // 32-bit offset limits the launchers check below hold for both tensors alike)
    k.seg_b = h->seg_b;
    for (int i = 0; i < BMC_MAX_SRC; ++i) k.seg_delta[i] = i < h->nsrc ? h->src_seg_delta[i] : 0;
    k.res_seg_delta = h->residual.ptr ? h->residual_seg_delta : 0;
    k.mask_seg_delta = h->mask.ptr ? h->mask_seg_delta : 0;
    {
        auto seg_ok = [&](const bmc_src_t& s, long long delta, long long given, const char* what) -> bool {
            if (given != delta) { bmc_set_error("bmc_conv: segment delta on an absent operand (%s)", what); return false; }
            if (delta == 0) return true;
            if (h->seg_b < 1 || h->seg_b >= h->B) {
                bmc_set_error("bmc_conv: %s has a segment delta but seg_b=%d is not in [1, B=%d)", what, h->seg_b, h->B);
                return false;
            }
            if (s.batch_shift != 0 || s.batch_mod < h->B) {
                bmc_set_error("bmc_conv: %s: a batch shift / modulus (%d / %d) cannot be combined with a batch segment", what,
                              s.batch_shift, s.batch_mod);
                return false;
            }
            if (delta % 4 != 0) { bmc_set_error("bmc_conv: %s: the segment's second tensor must be 16-byte aligned", what); return false; }
            return true;
        };
        for (int i = 0; i < BMC_MAX_SRC; ++i)
            if (!seg_ok(h->src[i < h->nsrc ? i : 0], k.seg_delta[i], h->src_seg_delta[i], "a source")) return -1;
        if (!seg_ok(h->residual, k.res_seg_delta, h->residual_seg_delta, "the residual")) return -1;
        if (!seg_ok(h->mask, k.mask_seg_delta, h->mask_seg_delta, "the mask")) return -1;
        BMC_CHECK_ARG(h->seg_b == 0 || (h->seg_b >= 1 && h->seg_b < h->B), "bmc_conv: seg_b=%d is not in [1, B=%d)", h->seg_b, h->B);
        // (the direct, bf16-plane and 1x1 kernels know no segment: refused here, in front of all of them)
        BMC_CHECK_ARG(!conv_has_segment(k) || h->math == BMC_MATH_FP32_WINO || h->math == BMC_MATH_FP32_WINO4,
                      "bmc_conv: batch segments are served by the Winograd kernels only (math %d given)", h->math);
    }
    // tile shape: 8x16 px x 128 ch when that fills the chip; small problems get 4-row tiles and/or 64-channel tiles so
    // that 2-4x as many workgroups share the work (a workgroup's K loop is serial: its latency is the launch's latency)
    const int cus = bmc_num_cus();
    int BN = h->Coutpad == 32 ? 32 : 128, THv = 8;
    auto count = [&](int th, int bn) {
        return (long long)h->B * ((h->W + TW - 1) / TW) * ((h->H + th - 1) / th) * (h->Coutpad / bn);
    };
    if (BN == 128 && count(8, 128) < 2ll * cus) {
        THv = 4;
        if (count(4, 128) < 2ll * cus) BN = 64;
    }
    k.tiles_x = (h->W + TW - 1) / TW; k.tiles_y = (h->H + THv - 1) / THv;
    k.ntn = h->Coutpad / BN;
    k.nchunks = ktot / CK;
    const long long ntiles = count(THv, BN);
    BMC_CHECK_ARG(ntiles < (1ll << 31), "bmc_conv: too many tiles");
    k.ntiles = (int)ntiles;
    BMC_CHECK_ARG(h->math == BMC_MATH_FP32 || h->math == BMC_MATH_BF16 || h->math == BMC_MATH_BF16X6 || h->math == BMC_MATH_FP32_WINO ||
                      h->math == BMC_MATH_FP32_WINO4,
                  "bmc_conv: unknown math mode %d", h->math);
    if (h->math == BMC_MATH_FP32_WINO) {
        BMC_CHECK_ARG(h->taps == 9 && h->Coutpad % 128 == 0, "bmc_conv: the Winograd path serves 3x3 taps with Coutpad a multiple of 128");
        const int rc = bmc_conv_wino_launch(k, cus, (hipStream_t)stream);
        if (rc) return rc;
        BMC_CHECK_LAUNCH("bmc_conv (winograd)");
        return 0;
    }
    if (h->math == BMC_MATH_FP32_WINO4) {
        BMC_CHECK_ARG(h->taps == 9 && h->Coutpad % 128 == 0, "bmc_conv: the Winograd path serves 3x3 taps with Coutpad a multiple of 128");
        const int rc = bmc_conv_wino4_launch(k, cus, (hipStream_t)stream);
        if (rc) return rc;
        BMC_CHECK_LAUNCH("bmc_conv (winograd F(4x4))");
        return 0;
    }
    if (h->math != BMC_MATH_FP32)
        return bmc_conv_bf_launch(k, h->taps, BN, THv, h->math == BMC_MATH_BF16 ? 1 : 3, cus, (hipStream_t)stream);
    static const bool no_conv1 = getenv("BMC_NO_CONV1") != nullptr;      // (A/B runs; read once, not per launch)
    if (h->taps == 1 && !no_conv1 && bmc_conv1_launch(k, cus, (hipStream_t)stream)) {
        BMC_CHECK_LAUNCH("bmc_conv (conv1)");
        return 0;
    }
    const int per_cu = (BN == 128 && THv == 8) ? 3 : 4;       // resident workgroups per CU (LDS / registers)
    const int max_blocks = cus * per_cu;
    dim3 grid((unsigned)(ntiles < max_blocks ? ntiles : max_blocks)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define BMC_LAUNCH_CONV(TAPS_, BN_, TH_) hipLaunchKernelGGL((conv_kernel<TAPS_, BN_, TH_>), grid, block, 0, st, k)
    if (h->taps == 9) {
        if (BN == 32) BMC_LAUNCH_CONV(9, 32, 8);
        else if (BN == 64) BMC_LAUNCH_CONV(9, 64, 4);
        else if (THv == 4) BMC_LAUNCH_CONV(9, 128, 4);
        else BMC_LAUNCH_CONV(9, 128, 8);
    } else {
        if (BN == 32) BMC_LAUNCH_CONV(1, 32, 8);
        else if (BN == 64) BMC_LAUNCH_CONV(1, 64, 4);
        else if (THv == 4) BMC_LAUNCH_CONV(1, 128, 4);
        else BMC_LAUNCH_CONV(1, 128, 8);
    }
#undef BMC_LAUNCH_CONV
    BMC_CHECK_LAUNCH("bmc_conv");
    return 0;
}
