// Weight gradient of a dense 3x3, 128 -> 128 channel convolution through the Winograd transform F(4x4, 3x3) on the fp32
// matrix cores (round 5): 36 multiplies per 4x4 output tile and channel pair -- 2.25 per output pixel, against 4 for the
// F(2x2) kernel of wino_wgrad.hip and 9 for the pixel-reduction GEMM of pgemm.hip:
//     dU[xi][nu][co][ci] = sum over tiles  dM[xi][nu][tile][co] * V[xi][nu][tile][ci],     dM = A dY A^T,  V = B^T d B,
//     dW = G^T dU G   (+ bias gradient = sum over tiles of dM[1][1] = the plain sum of the tile's 16 dY pixels),
// with d the 6x6 input patch and dY the 4x4 output-gradient patch of a tile (matrices: wino4.hip, the forward kernel).
// Numerics: 3.0e-6 rel-L2 per convolution against float64 (profiles/r04_wino_numerics.txt), contract 1e-3.
//
// Work split.  36 positions x 128 x 128 = 589 824 accumulators are eight workgroups' worth (144 per thread x 512 threads).
// What decides the split is the INPUT side: both operands are transformed per tile, and every workgroup that owns a slice of
// the output has to read and transform the pixels it needs.  A workgroup owns (xi group tg: xi in {3 tg .. 3 tg + 2}) x all six
// nu x (co half) x (ci half): it reads 64 channels of x (5 of the patch's 6 rows) and 64 channels of dY per tile -- 16 bytes per
// matrix-pipe cycle and CU, the least of the splits that fit the register file (4 positions x 128 x 128, the F(2x2) kernel's
// shape, would need 38) -- and with xi restricted to three rows the separable transforms cost each workgroup half of the full
// ones: the row combinations of three of B^T's / A's six rows, then the six column combinations of each.
// The tile axis is the reduction axis: `nsplit` workgroups per type share the stages in contiguous ranges and write partial
// sums, which wino4_wgrad_reduce_kernel adds in a fixed order and transforms to the 3x3 taps (deterministic).
//
// Stage = 4 horizontally adjacent tiles = 2 k-steps of v_mfma_f32_32x32x2_f32.  Wave (pg, cb, kb) owns the nine positions
// (3 xi) x (nu in {3 pg .. 3 pg + 2}) of the 32 x 32 block (co block cb, ci block kb): 9 x 16 accumulator registers, two waves
// per SIMD.  Per stage and wave: 18 MFMAs of 64 cycles, 18 ds_read2_b32 of operand fragments (lane -> channel l & 31, tile
// l >> 5 of the k-step: conflict-free).
// Raw pixels reach LDS by LDS-DMA, 39 pieces of 1 KB per stage, piece w + 8 j on wave w (five each, wave 7 four): no staging
// registers.  Inside the image a piece is "scalar base of the stage + a per-lane offset that never changes"; stages that touch the
// image border take a slower path (clamped per-lane addresses computed once per stage; the quads of out-of-image pixels are
// overwritten with zeros once landed) so that the transforms never see the border.
// LDS budget (160 KB): two raw buffers of 39 KB + two transformed images of 36 KB = 150 KB; one barrier per stage.
// Stage pipeline (round 7).  In stage s every wave multiplies stage s, transforms its share of stage s + 1 and requests its
// pieces of stage s + 2, all of it placed BETWEEN its own MFMAs by a compile-time timetable (sched_barrier fences): its DMA pieces
// behind MFMAs 0, 2, 4, 6, 8; the LDS reads of patch column c behind MFMA c, the column's combination three MFMAs later, the
// along-the-row combinations and the LDS writes behind MFMAs 10, 12, 14.  The transform is shared by all eight waves, one item
// (tile, channel pair) per lane: wave w takes tiles {0, 1} (w < 4) or {2, 3} of role w & 3 -- 0 the lone xi row of x (xi = 0 / 5),
// 1 / 2 sum / difference of the two xi rows that share their sub-sums (1, 2 / 3, 4), 3 all three xi of dY -- and the six (four)
// column chains of a lane are independent, so no gap holds more than a few dependent instructions.  Waves are specialised by
// role at compile time (no branches in the MFMA stream); the loop has three forms (request + transform, transform only, last).
// The end-of-stage vmcnt(0) follows the stage's last MFMA: the pieces have had ten MFMA gaps to land.
// Partial sums leave in REGISTER order (one 1 KB store per accumulator quad: [split][type][wave][position][quad][lane][4]);
// the reduction kernel knows the MFMA's D layout and reads them back as 16-byte quads of four consecutive output channels.
#include "bmc_common.h"
#include "dma_ring.h"

namespace {

struct Wgrad4K {
    SrcDev a;            // dY  [B,H,W,128]
    SrcDev x;            // the convolution's input [B,H,W,128]
    int B, H, W;
    int TY, SX;          // tile rows per image, stages (groups of 4 tiles) per tile row
    int nstages, nsplit;
    float* part;         // [nsplit][36 positions][128 co][128 ci]
    float* bias_part;    // optional [nsplit][128]
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

// a wave-uniform pointer, made opaque (readfirstlane) so that it lives in an SGPR pair
__device__ __forceinline__ const float* uni(const float* p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<const float*>(((unsigned long long)hi << 32) | lo);
}

constexpr int NPW = 18;                     // positions per workgroup: 3 xi x 6 nu
constexpr int TS = 4;                       // tiles per stage
constexpr int CH = 64;                      // channels of each operand per workgroup
constexpr int PIMG = TS * CH;               // floats of one position's image: [4 tiles][64 channels]
constexpr int IMG = NPW * PIMG;             // one operand's transformed image of a stage (18 KB)
constexpr int SIMG = 2 * IMG;               // dM image, then V image
constexpr int XPC = 23, YPC = 16;           // DMA pieces (4 pixels x 64 channels = 1 KB) of the raw x strip (5 rows x 18 pixels: 90
                                            // of the 92 pixel slots used) and of the raw dY strip (4 rows x 16 pixels)
constexpr int RAWX = XPC * 256;             // floats
constexpr int RAWF = (XPC + YPC) * 256;     // floats per raw buffer (39 KB)
constexpr int NPC = XPC + YPC;
constexpr int PPW = 5;                      // pieces per wave: piece w + 8 j (wave 7: four -- there is no piece 39)
constexpr int LDSF = 2 * RAWF + 2 * SIMG;   // 153 600 bytes: 2 x 39 KB raw + 2 x 36 KB transformed (of 160 KB)
static_assert(LDSF * 4 <= 160 * 1024, "LDS budget");

// The stage's timetable, in gaps: gap g follows the wave's MFMA g of the stage (position g >> 1, k-step g & 1).
//   DMA piece j:                 gap dma_gap(j) = 2 j (NOTEBOOK.md R7.1 has the other timetables measured)
//   transform, patch column c:   LDS reads at gap c, the column's combination at gap c + 3 (the reads have had ~3 MFMA gaps),
//   transform, output step k:    gap 10 + 2 k (the along-the-row combinations and the LDS writes)
constexpr int dma_gap(const int j) { return 2 * j; }
constexpr int TR_READ = 0, TR_COMB = 3, TR_OUT = 10;

template <int I, int N>
struct W4gFor {     // compile-time loop: f(integral_constant<int, I>) for I = 0 .. N - 1 (the accumulators must stay in registers)
    template <class F>
    static __device__ __forceinline__ void run(F&& f) {
        f(std::integral_constant<int, I>{});
        W4gFor<I + 1, N>::run(f);
    }
};
template <int N>
struct W4gFor<N, N> {
    template <class F>
    static __device__ __forceinline__ void run(F&&) {}
};

// ROLE = wave & 3: which part of the next stage's transform this wave computes (see the file header)
template <int TG, int ROLE>
__device__ __forceinline__ void wgrad4_body(const Wgrad4K& a, float* const lds, const int split, const int chh, const int kh) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* const rawb = lds;
    float* const imgb = lds + 2 * RAWF;
    const unsigned lds_raw = lds_addr(rawb);

    // ---- consumer role: wave = (nu group pg, co block cb, ci block kb); lane -> channel l & 31 of the block, tile l >> 5 of a k-step
    const int pg = wave >> 2, cb = (wave >> 1) & 1, kb = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int aoff = 3 * pg * PIMG + lh * CH + 32 * cb + l31;             // + (6 u + j) * PIMG + 2 ks * CH
    const int boff = IMG + 3 * pg * PIMG + lh * CH + 32 * kb + l31;
    f32x16 acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    // ---- requests: every wave issues its pieces w + 8 j of the stage after next, one per timetable slot.  Inside the image a piece
    // is "scalar base of the stage + a per-lane offset that never changes" (poff); a border stage's clamped per-lane offsets are
    // computed once per stage in rq_begin, outside the MFMA stream (pof: the offsets of the stage being requested)
    unsigned poff[PPW];       // byte offset from the stage's base pixel (interior stages)
    unsigned pof[PPW];        // the offsets of the stage in flight
    unsigned pla[PPW];        // LDS byte address of the piece in raw buffer 0
    unsigned pxm = 0;         // bit j: piece j is an x piece
    auto piece_of = [&](const int j) { return min(wave + 8 * j, NPC - 1); };
    const bool has_last = wave + 8 * (PPW - 1) < NPC;
    // pixel slot (row r, column c) of this lane's quad of piece p; false: not a pixel (the last two slots of the x strip)
    auto slot_of = [&](const int p, int& r, int& c) __attribute__((always_inline)) {
        if (p < XPC) { const int q = 4 * p + (lane >> 4); r = q / 18; c = q - 18 * r; return q < 90; }
        const int q = 4 * (p - XPC) + (lane >> 4); r = q >> 4; c = q & 15;
        return true;
    };
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        const int p = piece_of(j);
        int r, c;
        const bool real = slot_of(p, r, c);
        poff[j] = real ? (unsigned)(((r * a.W + c) * 128 + (lane & 15) * 4) * 4) : 0u;
        pof[j] = poff[j];
        pla[j] = lds_raw + (unsigned)(p * 1024);
        pxm |= p < XPC ? 1u << j : 0u;
    }
    unsigned zm = 0;          // bit j: this lane's quad of piece j is a pixel outside the image (stage in flight)
    static_assert(PPW <= 32, "zm is a bit mask");

    const int per_img = a.TY * a.SX;
    const int st0 = (int)((long long)a.nstages * split / a.nsplit), st1 = (int)((long long)a.nstages * (split + 1) / a.nsplit);
    // (image, tile row, group of 4 tiles) of the next stage to request, advanced incrementally; per tile row: the image's base
    // pointers (channel half included), the first pixel of the two strips' first rows, "the rows touch the image border"
    int nb = st0 / per_img, nty, nsx;
    {
        const int r = st0 - nb * per_img;
        nty = r / a.SX; nsx = r - nty * a.SX;
    }
    nb = __builtin_amdgcn_readfirstlane(nb); nty = __builtin_amdgcn_readfirstlane(nty); nsx = __builtin_amdgcn_readfirstlane(nsx);
    const float* xbat = nullptr;
    const float* ybat = nullptr;
    const float* xrow = nullptr;
    const float* yrow = nullptr;
    bool rowborder = false;
    auto row_setup = [&]() __attribute__((always_inline)) {
        xbat = uni(src_batch_ptr(a.x, nb) + kh * CH);
        ybat = uni(src_batch_ptr(a.a, nb) + chh * CH);
        const int y0 = 4 * nty - 1 + TG;                               // first staged patch row (TG = 1: patch rows 1..5)
        rowborder = y0 < 0 || y0 + 4 >= a.H;
        xrow = xbat + (long long)y0 * a.W * 128;                       // (only used when the rows are inside the image)
        yrow = ybat + (long long)(4 * nty) * a.W * 128;
    };
    row_setup();

    // rq_begin fixes the stage to request (scalar state, border offsets) and advances the cursor; rq_piece(j) issues piece j into
    // the raw buffer rq_begin named
    const float* rq_xs = nullptr;
    const float* rq_ys = nullptr;
    unsigned rq_lo = 0;
    auto rq_begin = [&](const int rb) __attribute__((always_inline)) {
        rq_lo = (unsigned)(rb * RAWF * 4);
        const int y0 = 4 * nty - 1 + TG, x0 = 16 * nsx - 1;
        const bool border = rowborder || nsx == 0 || x0 + 17 >= a.W;
        // interior: base = the strip's first pixel; border: base = the image (per-lane offsets are absolute then)
        rq_xs = border ? xbat : xrow + x0 * 128;
        rq_ys = border ? ybat : yrow + (x0 + 1) * 128;
        zm = 0;
        if (border) {
            asm volatile("; image border" ::: "memory");
#pragma unroll
            for (int j = 0; j < PPW; ++j) {
                const bool isx = (pxm >> j) & 1;
                int r, c;
                const bool real = slot_of(piece_of(j), r, c);
                const int y = (isx ? y0 : y0 + 1 - TG) + r, x = (isx ? x0 : x0 + 1) + c;
                const bool inside = y >= 0 && y < a.H && x >= 0 && x < a.W;
                const int yc = min(max(y, 0), a.H - 1), xc = min(max(x, 0), a.W - 1);
                pof[j] = real ? (unsigned)(((yc * a.W + xc) * 128 + (lane & 15) * 4) * 4) : 0u;
                zm |= (real && !inside) ? (1u << j) : 0u;
            }
        } else {
#pragma unroll
            for (int j = 0; j < PPW; ++j) pof[j] = poff[j];
        }
        if (!has_last) zm &= ~(1u << (PPW - 1));
        if (++nsx == a.SX) {
            nsx = 0;
            if (++nty == a.TY) { nty = 0; ++nb; }
            row_setup();
        }
    };
    auto rq_piece = [&](const int j) __attribute__((always_inline)) {
        if (j == PPW - 1 && !has_last) return;
        dma16_sgpr<1>(((pxm >> j) & 1) ? rq_xs : rq_ys, pof[j], pla[j] + rq_lo);
    };
    // after the requests have landed, before the barrier that publishes them: pixels outside the image become zeros
    auto patch = [&](const int rb) __attribute__((always_inline)) {
        if (__builtin_amdgcn_ballot_w64(zm != 0) == 0) return;
#pragma unroll
        for (int j = 0; j < PPW; ++j)
            if ((zm >> j) & 1) *reinterpret_cast<f32x4*>(rawb + (pla[j] - lds_raw) / 4 + rb * RAWF + lane * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    };

    // ---- transform of the next stage: item = (tile pt, channel pair cp), one per lane; wave w and w + 4 take tiles {0, 1} / {2, 3}.
    //   ROLE 0: the lone xi row of x: xi = 0 = (4 0 -5 0 1 0) on patch rows 0, 2, 4; xi = 5 = (0 4 0 -5 0 1) on patch rows 1, 3, 5 --
    //           staged rows 0, 2, 4 either way;
    //   ROLE 1 / 2: sum / difference of the two xi rows on patch rows 1..4 (staged rows 1 - TG ..): xi = 1, 2 = (r4 - 4 r2) +- (r3 - 4 r1);
    //           xi = 3, 4 = (r4 - r2) +- 2 (r3 - r1);
    //   ROLE 3: all three xi of dY: (y0, (y0 + y2) +- (y1 + y3)) or ((y0 + 4 y2) +- 2 (y1 + 4 y3), y3).
    // Then along the row: B^T (x) or A (dY) on the six / four column values.  The pieces are placed in the MFMA stream by the
    // timetable above; every lane's column chains are independent of each other.
    const int pt = 2 * (wave >> 2) + (lane >> 5), cp = lane & 31;
    constexpr int NK = ROLE == 0 ? 3 : 4;                                   // rows read per patch column
    constexpr int NC = ROLE == 3 ? 4 : 6;                                   // patch columns
    constexpr int KS = ROLE == 0 ? 2 * 18 * CH : (ROLE == 3 ? 16 * CH : 18 * CH);
    const int tsrc = (ROLE == 0 ? 4 * pt * CH : (ROLE == 3 ? RAWX + 4 * pt * CH : ((1 - TG) * 18 + 4 * pt) * CH)) + 2 * cp;
    const int tdst = (ROLE == 3 ? 0 : IMG + (ROLE == 0 ? (TG == 0 ? 0 : 2) : (TG == 0 ? 1 : 0) + (ROLE == 2 ? 1 : 0)) * 6 * PIMG) + pt * CH + 2 * cp;
    f32x2 td[NC][NK];          // the column's reads
    f32x2 tw[3][NC];           // combined columns (x roles: tw[0]; dY: the three xi rows)
    f32x2 bsum = {0.f, 0.f};
    auto ld2 = [](const float* p) __attribute__((always_inline)) { return *reinterpret_cast<const f32x2*>(p); };
    auto st2 = [](float* p, const f32x2 v) __attribute__((always_inline)) { *reinterpret_cast<f32x2*>(p) = v; };
    // the transform's share of gap G (compile time)
    auto tgap = [&](auto gc, const float* const raw, float* const img) __attribute__((always_inline)) {
        constexpr int G = decltype(gc)::value;
        constexpr int cr = G - TR_READ, cc = G - TR_COMB;
        if constexpr (cr >= 0 && cr < NC) {
#pragma unroll
            for (int k = 0; k < NK; ++k) td[cr][k] = ld2(raw + tsrc + k * KS + cr * CH);
        }
        if constexpr (cc >= 0 && cc < NC) {
            const f32x2* const d = td[cc];
            if constexpr (ROLE == 0) {
                tw[0][cc] = 4.f * d[0] - 5.f * d[1] + d[2];
            } else if constexpr (ROLE < 3) {
                constexpr float al = TG == 0 ? -4.f : -1.f;
                constexpr float ga = (TG == 0 ? 1.f : 2.f) * (ROLE == 2 ? -1.f : 1.f);
                tw[0][cc] = (d[3] + al * d[1]) + ga * (d[2] + al * d[0]);
            } else {
                constexpr float ka = TG == 0 ? 1.f : 4.f, la = TG == 0 ? 1.f : 2.f;
                const f32x2 p = d[0] + ka * d[2], q = d[1] + ka * d[3];
                if (TG == 0) { tw[0][cc] = d[0]; tw[1][cc] = p + la * q; tw[2][cc] = p - la * q; }
                else { tw[0][cc] = p + la * q; tw[1][cc] = p - la * q; tw[2][cc] = d[3]; }
            }
        }
        constexpr int ko = G - TR_OUT;
        if constexpr (ko >= 0 && ko < 6 && (ko & 1) == 0) {
            constexpr int k = ko >> 1;
            if constexpr (ROLE < 3) {
                // B^T along a row of six: (4 0 -5 0 1 0) (0 -4 -4 1 1 0) (0 4 -4 -1 1 0) (0 -2 -1 2 1 0) (0 2 -1 -2 1 0) (0 4 0 -5 0 1)
                const f32x2* const w = tw[0];
                float* const dst = img + tdst;
                if (k == 0) {
                    st2(dst, 4.f * w[0] - 5.f * w[2] + w[4]);
                    st2(dst + 5 * PIMG, 4.f * w[1] - 5.f * w[3] + w[5]);
                } else if (k == 1) {
                    const f32x2 ta = w[4] - 4.f * w[2], tb = w[3] - 4.f * w[1];
                    st2(dst + PIMG, ta + tb);
                    st2(dst + 2 * PIMG, ta - tb);
                } else {
                    const f32x2 tc = w[4] - w[2], te = w[3] - w[1];
                    st2(dst + 3 * PIMG, tc + 2.f * te);
                    st2(dst + 4 * PIMG, tc - 2.f * te);
                }
            } else {
                // A along a row of four: (1 0 0 0) (1 1 1 1) (1 -1 1 -1) (1 2 4 8) (1 -2 4 -8) (0 0 0 1), on xi row k of the group
                const f32x2* const w = tw[k];
                float* const dst = img + tdst + 6 * k * PIMG;
                const f32x2 s = w[0] + w[2], t = w[1] + w[3], p = w[0] + 4.f * w[2], q = w[1] + 4.f * w[3];
                const f32x2 m1 = s + t;
                st2(dst, w[0]);
                st2(dst + PIMG, m1);
                st2(dst + 2 * PIMG, s - t);
                st2(dst + 3 * PIMG, p + 2.f * q);
                st2(dst + 4 * PIMG, p - 2.f * q);
                st2(dst + 5 * PIMG, w[3]);
                if (TG == 0 && k == 1) bsum += m1;         // xi = 1, nu = 1: the sum of the tile's 16 dY pixels
            }
        }
    };

    // ---- one stage: 9 positions x 2 k-steps of v_mfma_f32_32x32x2_f32 on the stage's images, the timetable's pieces in the gaps.
    // The operand fragments of position i + 2 are requested before the MFMAs of position i are issued (a ring of three register
    // sets): no MFMA waits for an LDS round trip.  REQ: there is a stage after next to request; MORE: a next stage to transform
    auto stage = [&](const int it, auto reqc, auto morec) __attribute__((always_inline)) {
        constexpr bool REQ = decltype(reqc)::value, MORE = decltype(morec)::value;
        const float* const img = imgb + (it & 1) * SIMG;
        const float* const traw = rawb + ((it + 1) & 1) * RAWF;
        float* const timg = imgb + ((it + 1) & 1) * SIMG;
        if (REQ) rq_begin(it & 1);
        float af[3][2], bf[3][2];
        auto frag = [&](const int i) __attribute__((always_inline)) {
            const int u = i / 3, j = i - 3 * u, sl = i % 3;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                af[sl][ks] = img[aoff + (6 * u + j) * PIMG + 2 * ks * CH];
                bf[sl][ks] = img[boff + (6 * u + j) * PIMG + 2 * ks * CH];
            }
        };
        __builtin_amdgcn_sched_barrier(0);
        frag(0);
        frag(1);
        W4gFor<0, 9>::run([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = decltype(ic)::value;
            __builtin_amdgcn_sched_barrier(0);
            if (i + 2 < 9) frag(i + 2);
            __builtin_amdgcn_sched_barrier(0);
            W4gFor<0, 2>::run([&](auto kc) __attribute__((always_inline)) {
                constexpr int ks = decltype(kc)::value, g = 2 * i + ks;
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i % 3][ks], bf[i % 3][ks], acc[i], 0, 0, 0);
                if (REQ) {
#pragma unroll
                    for (int j = 0; j < PPW; ++j)
                        if (dma_gap(j) == g) rq_piece(j);
                }
                if (MORE) tgap(std::integral_constant<int, g>{}, traw, timg);
                __builtin_amdgcn_sched_barrier(0);
            });
        });
        dma_wait<0>();
        if (REQ) patch(it & 1);
        ring_publish();
    };

    // ---- prologue: stage st0 raw -> image 0, stage st0 + 1 requested
    const int n = st1 - st0;
    if (n <= 0) return;
    rq_begin(0);
#pragma unroll
    for (int j = 0; j < PPW; ++j) rq_piece(j);
    dma_wait<0>();
    patch(0);
    ring_publish();
    if (n > 1) {
        rq_begin(1);
#pragma unroll
        for (int j = 0; j < PPW; ++j) rq_piece(j);
    }
    W4gFor<0, 18>::run([&](auto gc) __attribute__((always_inline)) { tgap(gc, rawb, imgb); });
    dma_wait<0>();
    if (n > 1) patch(1);
    ring_publish();
    // ---- stage it: multiply stage it, transform stage it + 1, request stage it + 2 (into the raw buffer stage it was made from)
    using T_ = std::true_type;
    using F_ = std::false_type;
    int it = 0;
    for (; it + 2 < n; ++it) stage(it, T_{}, T_{});
    if (it + 1 < n) stage(it++, F_{}, T_{});
    stage(it, F_{}, F_{});

    // ---- partial sums in register order: part[split][type][wave][position 3 u + j][quad m][lane][4] -- D row 8 m + 4 (l >> 5) + e
    // (co), column l & 31 (ci), e = 0..3: one coalesced 1 KB store per accumulator quad
    {
        float* const P = a.part + ((((long long)split * 8 + (TG * 4 + chh * 2 + kh)) * 8 + wave) * 9) * 1024 + lane * 4;
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int m = 0; m < 4; ++m)
                stg16(P + (i * 4 + m) * 256, f32x4{acc[i][4 * m], acc[i][4 * m + 1], acc[i][4 * m + 2], acc[i][4 * m + 3]});
    }
    if (TG == 0 && kh == 0 && a.bias_part) {      // bias partial: the 4 tile slots added through LDS (the loop ended on a barrier)
        if (ROLE == 3) *reinterpret_cast<f32x2*>(lds + pt * CH + 2 * cp) = bsum;      // (the dY waves 3 / 7: tiles {0, 1} / {2, 3})
        __syncthreads();
        if (tid < CH) a.bias_part[(long long)split * 128 + 64 * chh + tid] = (lds[tid] + lds[CH + tid]) + (lds[2 * CH + tid] + lds[3 * CH + tid]);
    }
}

template <int TG>
__device__ __forceinline__ void wgrad4_role(const Wgrad4K& a, float* const lds, const int split, const int chh, const int kh) {
    switch (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 3) {
        case 0: wgrad4_body<TG, 0>(a, lds, split, chh, kh); break;
        case 1: wgrad4_body<TG, 1>(a, lds, split, chh, kh); break;
        case 2: wgrad4_body<TG, 2>(a, lds, split, chh, kh); break;
        default: wgrad4_body<TG, 3>(a, lds, split, chh, kh); break;
    }
}

__global__ __launch_bounds__(512, 2) void wino4_wgrad_kernel(const Wgrad4K a) {
    __shared__ __attribute__((aligned(16))) float lds[LDSF];
    // workgroup -> (type, split): the eight types of a split read the same pixels -- on the same XCD (same L2) when the split
    // count allows (consecutive workgroup ids go round the 8 XCDs)
    int type, split;
    if ((a.nsplit & 7) == 0) {
        const int j = blockIdx.x >> 3;
        type = j & 7; split = (j >> 3) * 8 + (blockIdx.x & 7);
    } else {
        type = blockIdx.x & 7; split = blockIdx.x >> 3;
    }
    const int chh = (type >> 1) & 1, kh = type & 1;
    if (type & 4) wgrad4_role<1>(a, lds, split, chh, kh);
    else wgrad4_role<0>(a, lds, split, chh, kh);
}

// dW[co][k0 + ci][3][3] (+)= G^T (sum over splits of dU) G, db[co] (+)= sum of the bias partials.
// 512 workgroups of 288 threads (+ one for the bias).  Workgroup (c, r): c = (chh, kh, cb, kb) names a 32 x 32 accumulator block of
// every position, r eight consecutive quads of it (quad m = r >> 3, lanes 8 (r & 7) .. + 7: four co x eight ci).  Phase 1: thread
// (position p, quad) adds the 16-byte quads of all splits in split order, eight loads in flight.  Phase 2: thread (co, ci, tap)
// applies G^T . G over the 36 positions held in LDS, in the order the summation always had.  Deterministic.
constexpr int RED_THREADS = 288, RED_GROUPS = 512;
__global__ __launch_bounds__(RED_THREADS) void wino4_wgrad_reduce_kernel(const float* __restrict__ part, int nsplit, float* __restrict__ dw,
                                                                        int ldw, int k0, int accumulate, const float* __restrict__ bias_part,
                                                                        float* __restrict__ db) {
    constexpr long long SSTRIDE = 36ll * 16384;     // floats per split
    const int t = threadIdx.x;
    if ((int)blockIdx.x == RED_GROUPS) {            // bias: 128 channels, splits in order, eight loads in flight
        if (t >= 128) return;
        float s = 0.f;
        int i = 0;
        for (; i + 8 <= nsplit; i += 8) {
            float q[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) q[k] = bias_part[(long long)(i + k) * 128 + t];
#pragma unroll
            for (int k = 0; k < 8; ++k) s += q[k];
        }
        for (; i < nsplit; ++i) s += bias_part[(long long)i * 128 + t];
        db[t] = accumulate ? db[t] + s : s;
        return;
    }
    __shared__ f32x4 U[36][8];
    const int c = blockIdx.x >> 5, r = blockIdx.x & 31;
    const int chh = c >> 3, kh = (c >> 2) & 1, cb = (c >> 1) & 1, kb = c & 1;
    const int m = r >> 3, lane0 = 8 * (r & 7);
    {
        const int p = t >> 3, qi = t & 7;
        const int xi = p / 6, nu = p - 6 * xi;
        const int type = (xi / 3) * 4 + chh * 2 + kh, wv = (nu / 3) * 4 + cb * 2 + kb, a9 = 3 * (xi % 3) + nu % 3;
        const float* const ps = part + (((long long)type * 8 + wv) * 9 + a9) * 1024 + m * 256 + (lane0 + qi) * 4;
        f32x4 u = {0.f, 0.f, 0.f, 0.f};
        int s = 0;
        for (; s + 8 <= nsplit; s += 8) {
            f32x4 q[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) q[k] = ldg16(ps + (s + k) * SSTRIDE);
#pragma unroll
            for (int k = 0; k < 8; ++k) u += q[k];
        }
        for (; s < nsplit; ++s) u += ldg16(ps + s * SSTRIDE);
        U[p][qi] = u;
    }
    __syncthreads();
    // rows of G: (1/4 0 0) (-1/6 -1/6 -1/6) (-1/6 1/6 -1/6) (1/24 1/12 1/6) (1/24 -1/12 1/6) (0 0 1);
    // dW[i][j] = sum_xi,nu G[xi][i] G[nu][j] dU[xi][nu]
    const float G[6][3] = {{0.25f, 0.f, 0.f}, {-1.f / 6, -1.f / 6, -1.f / 6}, {-1.f / 6, 1.f / 6, -1.f / 6},
                           {1.f / 24, 1.f / 12, 1.f / 6}, {1.f / 24, -1.f / 12, 1.f / 6}, {0.f, 0.f, 1.f}};
    const int e = t / 72, r2 = t - 72 * e, qi = r2 / 9, tap = r2 - 9 * qi, ti = tap / 3, tj = tap - 3 * ti;
    float o = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {          // eight interleaved partial sums over the positions, then added in order
        float tk = 0.f;
#pragma unroll
        for (int p = k; p < 36; p += 8) {
            const int xi = p / 6, nu = p - 6 * xi;
            float gi = 0.f, gj = 0.f;
#pragma unroll
            for (int q = 0; q < 3; ++q) { gi = q == ti ? G[xi][q] : gi; gj = q == tj ? G[nu][q] : gj; }
            tk += (gi * gj) * U[p][qi][e];
        }
        o += tk;
    }
    const int co = 64 * chh + 32 * cb + 8 * m + 4 * (lane0 >> 5) + e, ci = 64 * kh + 32 * kb + (lane0 & 31) + qi;
    float* const d = dw + ((long long)co * ldw + k0 + ci) * 9 + tap;
    *d = accumulate ? *d + o : o;
}

}  // namespace

static long long w4g_stages(int B, int H, int W) { return (long long)B * ((H + 3) / 4) * (((W + 3) / 4 + TS - 1) / TS); }

extern "C" int bmc_wgrad_wino4_nsplit(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    const long long stages = w4g_stages(B, H, W);
    const int per_type = bmc_num_cus() / 8 > 0 ? bmc_num_cus() / 8 : 1;
    return (int)(stages < per_type ? stages : per_type);
}

extern "C" int bmc_wgrad_wino4(const bmc_src_t* dy, const bmc_src_t* x, int B, int H, int W, int nsplit, float* part,
                               float* bias_part, bmc_stream_t s) {
    BMC_CHECK_ARG(dy && x && part && dy->ptr && x->ptr, "bmc_wgrad_wino4: null argument");
    BMC_CHECK_ARG(dy->nch == 128 && x->nch == 128, "bmc_wgrad_wino4: both operands must be 128-channel windows (got %d, %d)", dy->nch,
                  x->nch);
    BMC_CHECK_ARG(dy->pix_stride == 128 && x->pix_stride == 128, "bmc_wgrad_wino4: both operands must be dense in the channel axis "
                  "(pix_stride 128; got %d, %d)", dy->pix_stride, x->pix_stride);
    BMC_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && (long long)H * W * 128 < (1ll << 29), "bmc_wgrad_wino4: bad geometry");
    Wgrad4K k;
    k.a = to_dev(*dy); k.x = to_dev(*x);
    k.B = B; k.H = H; k.W = W;
    k.TY = (H + 3) / 4; k.SX = ((W + 3) / 4 + TS - 1) / TS;
    const long long stages = w4g_stages(B, H, W);
    BMC_CHECK_ARG(stages < (1ll << 31), "bmc_wgrad_wino4: too many tiles");
    BMC_CHECK_ARG(nsplit >= 1 && nsplit <= stages, "bmc_wgrad_wino4: nsplit must be in [1, %lld]", stages);
    k.nstages = (int)stages; k.nsplit = nsplit;
    k.part = part; k.bias_part = bias_part;
    hipLaunchKernelGGL(wino4_wgrad_kernel, dim3((unsigned)nsplit * 8), dim3(512), 0, (hipStream_t)s, k);
    BMC_CHECK_LAUNCH("bmc_wgrad_wino4");
    return 0;
}

extern "C" int bmc_wgrad_wino4_reduce(const float* part, int nsplit, float* dw, int ldw, int k0, int accumulate,
                                      const float* bias_part, float* db, bmc_stream_t s) {
    BMC_CHECK_ARG(part && dw && nsplit >= 1, "bmc_wgrad_wino4_reduce: bad arguments");
    BMC_CHECK_ARG(ldw >= 128 && k0 >= 0 && k0 + 128 <= ldw, "bmc_wgrad_wino4_reduce: columns [k0, k0 + 128) must lie inside the %d input "
                  "channels of the weight tensor", ldw);
    BMC_CHECK_ARG((bias_part == nullptr) == (db == nullptr), "bmc_wgrad_wino4_reduce: bias_part and db go together");
    hipLaunchKernelGGL(wino4_wgrad_reduce_kernel, dim3(RED_GROUPS + (bias_part ? 1 : 0)), dim3(RED_THREADS), 0, (hipStream_t)s, part, nsplit, dw, ldw, k0,
                       accumulate, bias_part, db);
    BMC_CHECK_LAUNCH("bmc_wgrad_wino4_reduce");
    return 0;
}
