/*
 * bmc_hip.h -- C ABI of libbmc_hip.so, the MI355X (gfx950) kernel library behind
 * the BMCNet bilateral event-SR hot path.
 *
 * The reference (Lqm26/BMCNet-ESR) has no FFI: its hot path is a chain of ATen
 * calls issued from Python.  Each entry point below replaces the
 * ATen call sites cited next to it; the Python host side
 * (bmcnet-esr_amd/bmc_hip) binds them with ctypes and wraps fwd/bwd pairs in
 * torch.autograd.Function objects behind the reference's own nn.Module
 * signatures.
 *
 * Conventions
 *  - plain pointers + sizes only; every pointer is DEVICE memory unless a
 *    parameter is documented as a host struct;
 *  - activations are fp32 NHWC: element (b,y,x,c) of a tensor lives at
 *    ptr[b*batch_stride + (y*W + x)*pix_stride + c];
 *  - nothing allocates: workspaces are passed in;
 *  - every launch goes to the hipStream_t given (pass torch's current stream);
 *  - return 0 on success, <0 on error (bmc_last_error() has the text).
 */
#ifndef BMC_HIP_H
#define BMC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* bmc_stream_t; /* hipStream_t */

#define BMC_MAX_SRC 6
#define BMC_CK 16 /* channel granule: every source's nch is a multiple of 16 */

/* A channel-slice of an NHWC tensor used as one operand of a multi-source
 * convolution (what the reference builds with torch.cat, models/BMCNet.py:60-73,
 * models/submodules.py:63-64,75).  Batch index b of the launch reads batch
 * (b + batch_shift) % batch_mod of this tensor (shared / swapped operands of the
 * weight-shared twin branches). */
typedef struct bmc_src {
    const float* ptr;
    long long batch_stride; /* floats */
    int pix_stride;         /* floats */
    int nch;                /* channels consumed from ptr, multiple of 16 */
    int batch_shift;
    int batch_mod;          /* >= 1, or BMC_SRC_TABLE: `ptr` is a device table of per-image base pointers (bmc_ptr_table) */
} bmc_src_t;
/* batch_mod == BMC_SRC_TABLE: image b of the launch starts at ((const float* const*)ptr)[b] -- the images of one operand gathered
 * from several tensors (the uses of ONE weight by the weight-sharing blocks of a window reduced by one weight-gradient launch,
 * models/BMCNet.py:19-32); pix_stride / nch as usual, batch_stride / batch_shift unused. */
#define BMC_SRC_TABLE (-1)


/* ---- library ---- */
int bmc_version(void);
const char* bmc_last_error(void);
/* The ABI of this build as text, one record per line: every entry point's return and parameter types, every struct's size,
 * alignment and fields (offset, size, element type, array extents) and every numeric BMC_* constant of this header, as the
 * compiler that built the library saw them (csrc/abi.hip gives the record formats).  A binding is built from this text, not
 * from a second copy of this header.  The string lives as long as the library. */
const char* bmc_abi(void);
/* A new stream of the device's lowest priority (hipDeviceGetStreamPriorityRange), never destroyed by the library.  The training
 * step issues its weight-gradient kernels there (the reference has no counterpart: autograd runs train.py:233's backward on
 * one stream): they fill the CUs the data-gradient chain leaves idle without delaying it. */
int bmc_stream_create_low_priority(bmc_stream_t* out);

/* ---- event -> count image: dataloader/encodings.py:241-269,290-305 -------
 * events_to_channels() for `nframes` frames in one launch.  Frame f owns events
 * [offsets[f], offsets[f+1]) of xs/ys/ps (fp32, as event_formatting() leaves
 * them, dataloader/base_dataset.py:24-31) and writes out[f] = [2,H,W] fp32
 * (zero-filled here).  Bit-exact with the reference including its quirk: an
 * out-of-range event is dropped from channel 0, but its x,y are reset to 0 in
 * place so a NEGATIVE one lands on [H-1,0] of channel 1.  If mutate != 0 xs/ys
 * are updated in place as the reference does to its caller's tensors. */
int bmc_events_to_channels(float* xs, float* ys, const float* ps, const long long* offsets,
                           int nframes, int H, int W, float* out, int mutate, bmc_stream_t s);

/* The same two encoders for LARGE frames (the 720x960 ground-truth frames of the training step) without scattered global
 * float atomics: events are counting-sorted by row band (integer atomics on a small table), one workgroup per
 * (frame, band) accumulates its band of the count image in LDS and stores it once (that store is also the zero fill).
 * Same results bit for bit (integer-valued sums), same in-place side effect on xs / ys with mutate.  nevents =
 * offsets[nframes]; ws: 8-byte aligned workspace of bmc_events_binned_ws_bytes(nevents, nframes, H, W) bytes
 * ((frame, band) count table and cursors + 8 bytes per event).  W <= 16384. */
long long bmc_events_binned_ws_bytes(long long nevents, int nframes, int H, int W);
int bmc_events_to_channels_binned(float* xs, float* ys, const float* ps, const long long* offsets, long long nevents,
                                  int nframes, int H, int W, float* out, int mutate, void* ws, long long ws_bytes,
                                  bmc_stream_t s);
int bmc_encode_raw_events_binned(const short* xs, const short* ys, const double* ps, const long long* offsets,
                                 const unsigned char* flips, long long nevents, int nframes, int H, int W, float* out,
                                 void* ws, long long ws_bytes, bmc_stream_t s);

/* The torch-tensor encodings of the reference (no caller in the reference; they complete the encodings row):
 * events_to_image_torch (dataloader/encodings.py:16-73) on one event list -> out [H][W], or [H+1][W+1] for bilinear
 * interpolation with padding.  bilinear != 0: interpolate_to_image (:6-13), sub-pixel positions spread over the four
 * neighbours; bilinear == 0: img[ys.long(), xs.long()] += ps.  Out-of-range events are reset IN PLACE to (0, 0) with weight 0
 * (:33-38) -- xs, ys, ps are mutated like the reference's tensors.  The sums are taken in the order of the reference's CPU
 * index_put_(accumulate=True) (one pass per corner, events in order): deterministic and bit-identical to it.
 * ws: bmc_events_torch_ws_ints(n, H, W) ints.  bilinear without padding requires clip_out_of_range.
 * events_to_voxel_torch (:100-148), temporal_bilinear=True: out [bins][H][W]; ts sorted ascending and >= 0; zeros for
 * n <= 3 or all-zero timestamps (:121-122); xs, ys are reset in place by the first bin's call (ps is not touched). */
long long bmc_events_torch_ws_ints(long long n, int H, int W);
int bmc_events_to_image_torch(float* xs, float* ys, float* ps, long long n, int H, int W, int clip_out_of_range, int bilinear,
                              int padding, float* out, int* ws, bmc_stream_t s);
int bmc_events_to_voxel_torch(float* xs, float* ys, const float* ts, const float* ps, long long n, int bins, int H, int W,
                              float* out, int* ws, bmc_stream_t s);

/* events_to_voxel(): temporal-bilinear voxel grid [nframes][bins][H][W] (dataloader/encodings.py:272-287; ts already
 * normalised to [0,1] by event_formatting).  Same coordinate conventions and first-call side effect as above.  The
 * weights are arbitrary floats, so the order of summation is part of the result: a pixel's events are added in EVENT
 * ORDER, as the reference's sequential index_put_ does -- deterministic (no float atomics) and bit-identical to the
 * single-threaded reference.  nevents = offsets[nframes]; ws: workspace of 2*nframes*(H*W + 1) + nevents ints. */
int bmc_events_to_voxel(float* xs, float* ys, const float* ts, const float* ps, const long long* offsets,
                        long long nevents, int nframes, int bins, int H, int W, float* out, int mutate, int* ws,
                        bmc_stream_t s);

/* events_to_stack_no_polarity() (dataloader/encodings.py:202-238): `bins` temporal bins over one event window, each the
 * signed per-pixel sum of the polarities of its events at [(long) y, (long) x] (no vertical flip).  tstart / tend [bins]:
 * the float32 bin bounds ts[0] + delta_t*bi and tstart + delta_t, computed by the caller with the reference's float32
 * expressions; the bins' event ranges come from the reference's own binary search (:75-97, quirks included) run on
 * the device, into `ranges` [2*bins] ints.  If mutate != 0, out-of-range events covered by a bin get xs = ys = ps = 0 in
 * place, as the reference does to its caller's tensors.  Exact for +-1 polarities (integer-valued sums). */
int bmc_events_to_stack(float* xs, float* ys, const float* ts, float* ps, long long n, const float* tstart,
                        const float* tend, int bins, int H, int W, float* out, int* ranges, int mutate, bmc_stream_t s);

/* events_to_stack_polarity() (dataloader/encodings.py:151-199): as bmc_events_to_stack but two COUNT images per bin,
 * out [2][bins][H][W] = (positives, negatives), weights p*p.  The reference's first (positive) call of the first bin that
 * covers an event resets its out-of-range coordinates (in place, if mutate) and masks only that call: an out-of-range
 * negative event counts at [0,0] of the negative image, and an out-of-range event that a later, overlapping bin covers
 * again counts at [0,0] whatever its sign.  ps is never modified. */
int bmc_events_to_stack_polarity(float* xs, float* ys, const float* ts, const float* ps, long long n, const float* tstart,
                                 const float* tend, int bins, int H, int W, float* out, int* ranges, int mutate,
                                 bmc_stream_t s);

/* events_to_mask() (dataloader/encodings.py:308-332; the hot-pixel filter's input, dataloader/h5dataset.py:528-546):
 * out [H][W], out[(long) y][(long) x] = |p| of the LAST event (in order) that maps there -- index_put_(accumulate=False)
 * semantics, made deterministic with an integer atomicMax over event indices (ws: H*W ints).  Out-of-range events
 * count as (0, 0) with p = 0; if mutate != 0 their xs / ys / ps are zeroed in place as the reference does. */
int bmc_events_to_mask(float* xs, float* ys, float* ps, long long n, int H, int W, float* out, int* ws, int mutate,
                       bmc_stream_t s);

/* Sequence encoder on raw dataset columns: what H5Dataset.__getitem__ does per frame on the CPU
 * (dataloader/h5dataset.py:261-316: get_events :407-414 -> augment_event :559-578 -> event_formatting
 * base_dataset.py:24-31 -> events_to_channels), for all frames of a batch in one launch.
 * xs/ys int16, ps float64 (generate_dataset/tools/event_packagers.py:128-156); flips[f] bit0 horizontal
 * (x = W-1-x), bit1 vertical (y = H-1-y), bit2 polarity (p = -p); flips NULL = no augmentation. */
int bmc_encode_raw_events(const short* xs, const short* ys, const double* ps, const long long* offsets,
                          const unsigned char* flips, int nframes, int H, int W, float* out, bmc_stream_t s);

/* ---- weight packing ------------------------------------------------------
 * Conv weights [G][Cout][Cin][taps] (taps = kh*kw = 1 or 9; nn.Conv2d layout)
 * -> MFMA staging layout [G][Kpad/16][taps][Coutpad][16] where packed input
 * channel k holds reference input channel kmap[k] (or zero when kmap[k] < 0).
 * transpose != 0 builds the data-gradient operator instead: output channels =
 * packed k (Kpad rounded up to Coutpad_t), reduction over Cout, taps mirrored.
 * kmap: DEVICE array of Kpad ints (bmc_pack_weight*) or at least k0 + nk ints (the transposed packs), every entry < Cin;
 * kmap NULL is the implicit map k -> k for k < Cin and -1 (zero) for k >= Cin, in every pack below, forward and transposed. */
int bmc_pack_weight(const float* w, const int* kmap, int G, int Cout, int Cin, int taps,
                    int Kpad, int Coutpad, float* out, bmc_stream_t s);
int bmc_pack_weight_t(const float* w, const int* kmap, int G, int Cout, int Cin, int taps,
                      int k0, int nk, int nkpad, int Coutpad16, float* out, bmc_stream_t s);
/* Packed fp32 weights [nsteps][Coutpad][16] (nsteps = G * Kpad/16 * taps) -> `planes` bf16 planes
 * [nsteps][planes][Coutpad][16] for bmc_conv with math = BMC_MATH_BF16 (planes 1) / BMC_MATH_BF16X6 (planes 3);
 * `out` holds nsteps*planes*Coutpad*16 bf16 values (2 bytes each); inside a 32-byte row the two 16-byte halves are
 * swapped when (row & 16), the kernel's conflict-free LDS image (the weight stream is a linear LDS-DMA copy of it). */
#define BMC_MATH_FP32 0
#define BMC_MATH_BF16 1
#define BMC_MATH_BF16X6 3
#define BMC_MATH_FP32_WINO 4 /* bmc_conv only: fp32 MFMA through the Winograd transform F(2x2, 3x3), below */
#define BMC_MATH_FP32_WINO4 5 /* bmc_conv only: the same through F(4x4, 3x3) (bmc_pack_weight_wino4) */
int bmc_split_weight(const float* packed, void* out, long long nsteps, int Coutpad, int planes, bmc_stream_t s);

/* Conv weights [G][Cout][Cin][3][3] -> the TRANSFORMED weights U = G g G^T of Winograd's F(2x2, 3x3) minimal filtering
 * (16 values per (co, ci) pair instead of 9), in the streaming order of bmc_conv with math = BMC_MATH_FP32_WINO:
 * [G][Kpad/16][4 (xi)][4 (nu)][Coutpad][16]; the four 4-float quads of a 16-float row are XOR-swizzled: quad q of row r is stored
 * at quad q ^ SWZ[(r >> 2) & 3] with SWZ = {0, 2, 3, 1} (csrc/dma_ring.h::swz, the kernels' conflict-free LDS image).
 *   transposed == 0: rows = output channels (Coutpad: multiple of 128), K = packed input channels through kmap (as
 *                    bmc_pack_weight);  w_group_stride of the launch = Kpad * Coutpad * 16 floats;
 *   transposed != 0: the data-gradient operator w.r.t. packed source channels [k0, k0 + nk): rows = those channels (padded
 *                    to Coutpad), K = the Cout output channels (padded to Kpad), taps mirrored (as bmc_pack_weight_t). */
int bmc_pack_weight_wino(const float* w, const int* kmap, int G, int Cout, int Cin, int Kpad, int Coutpad, int transposed,
                         int k0, int nk, float* out, bmc_stream_t s);

/* Rows per workgroup tile (8 or 4) that bmc_conv with math = BMC_MATH_FP32_WINO uses for a launch of B images of H x W pixels and
 * Coutpad output channels on a device of `cus` compute units (<= 0: 256): 4 where the 8 x 16-pixel tiling leaves CUs without a
 * tile and the 4 x 16 one does not (small frames).  The host's routing rule (bmc_hip/ops.py::wino_ok) counts tiles with it. */
int bmc_conv_wino_rows(int B, int H, int W, int Coutpad, int cus);

/* The same for F(4x4, 3x3) (36 values per (co, ci) pair, made in double and rounded once; points 0, +-1, +-2, inf), in the
 * streaming order of bmc_conv with math = BMC_MATH_FP32_WINO4: [G][Coutpad/128][Kpad/16][8 (wave)][36 (position)][64 (lane)][4],
 * lane l of wave w = row 128 ntile + 16 w + (l & 15), channels 16 chunk + 4 (l >> 4) + 0..3 -- the MFMA A-operand image a wave
 * loads with one 1 KB instruction per position.  Arguments as bmc_pack_weight_wino; w_group_stride of the launch =
 * Kpad * Coutpad * 36 floats.  Replaces the weight operand of the 3x3 F.conv2d calls at models/submodules.py:31-35 (the
 * residual blocks: 100 of the 103 3x3 convolutions of a window, models/BMCNet.py:19-32) and models/BMCNet.py:64-82. */
int bmc_pack_weight_wino4(const float* w, const int* kmap, int G, int Cout, int Cin, int Kpad, int Coutpad, int transposed,
                          int k0, int nk, float* out, bmc_stream_t s);

/* ---- implicit-GEMM convolution (fp32 MFMA) -------------------------------
 * Replaces F.conv2d at models/submodules.py:25-26,33-34,44-53,63-67,75 and
 * models/BMCNet.py:40-53,64-82 together with the torch.cat / relu / residual
 * add around them, and torch.bmm(softmax, v) at models/submodules.py:72-73
 * (a 1x1 convolution with per-sample weights).  Also the data gradient of all
 * of these (same kernel, transposed weights).
 *   out[b,y,x,co] = epi( sum_{tap,k} W[g][k][tap][co] * cat(src)[b, y+dy, x+dx, k] + bias[g][co] )
 *   epi(v) = relu? max(v,0) : v, after adding residual[b,y,x,co] if given;
 *   g = b / batch_per_group. */
typedef struct bmc_conv_args {
    int nsrc;
    bmc_src_t src[BMC_MAX_SRC];
    const void* wpacked;        /* from bmc_pack_weight (math 0) or bmc_split_weight of it (math 1, 3) */
    const float* bias;          /* [G][Cout] or NULL */
    long long w_group_stride;   /* 32-bit words between groups in wpacked (math 0: floats; math 1 / 3: floats * planes / 2) */
    int bias_group_stride;
    int batch_per_group;        /* >= 1 */
    float* out;
    long long out_batch_stride;
    int out_pix_stride;
    int B, H, W;
    int Cout, Coutpad;          /* Coutpad: multiple of 32 (of 128 when > 32) */
    int taps;                   /* 1 or 9 */
    int relu;
    bmc_src_t residual;         /* ptr NULL -> none; nch ignored */
    bmc_src_t mask;             /* ptr NULL -> none; out = mask > 0 ? v : 0 (ReLU backward) */
    int accumulate;             /* out += v */
    int math;                   /* BMC_MATH_FP32 (0): v_mfma_f32_32x32x2_f32 on the fp32 operands;
                                   BMC_MATH_BF16 (1): operands rounded to bf16, fp32 accumulate (v_mfma_f32_32x32x16_bf16);
                                   BMC_MATH_BF16X6 (3): each fp32 operand split exactly into three bf16 planes, six plane
                                   products with fp32 accumulate -- fp32-equivalent (dropped terms ~ one fp32 rounding per product);
                                   BMC_MATH_FP32_WINO (4): taps = 9, Coutpad % 128 == 0, wpacked from bmc_pack_weight_wino: fp32 MFMA
                                   on Winograd-transformed operands, F(2x2, 3x3): 16 instead of 36 multiplies per 2x2 output
                                   tile and channel pair, fp32 throughout (error vs float64 ~1.5x the direct fp32 kernel's) */
    /* Batch segment: one launch whose images come from TWO tensors of the same H, W, pixel stride and channel window (two
     * independent, equally shaped convolutions with their own weight groups sharing a launch without a torch.cat of the inputs).
     * seg_b = 0: none (every delta below must be 0).  1 <= seg_b < B: an operand with a non-zero delta reads launch images
     * b < seg_b from its descriptor as usual and images b >= seg_b at the address of image b PLUS its delta (floats, signed):
     * delta = (second tensor's image 0) - (descriptor's image seg_b).  Such an operand has batch_shift 0 and no wrapping
     * modulus (batch_mod >= B); operands with delta 0 are ordinary ones.  Served by the Winograd kernels (math 4, 5); every
     * other kernel of bmc_conv refuses a segmented launch. */
    int seg_b;
    long long src_seg_delta[BMC_MAX_SRC];
    long long residual_seg_delta;
    long long mask_seg_delta;
} bmc_conv_args_t;
int bmc_conv(const bmc_conv_args_t* host_args, bmc_stream_t s);

/* ---- pixel-reduction GEMM: weight gradients and channel Gram matrices ----
 *   C[g][tap][m][n] = sum_{b in group g} sum_{y,x} A[b,y,x,m] * cat(src)[b,y+dy,x+dx,n]
 * Replaces the weight-gradient half of conv backward (ATen autograd) and
 * torch.bmm(center, v) at models/submodules.py:69-70 (+ its backward).
 * Split over pixels: partial sums go to `slabs`
 * [nsplit][G][taps][Mpad][Npad] (Mpad/Npad = M/N rounded up to 32), which one of
 * the reduce calls below then sums (deterministic order).
 * nsplit may exceed the number of pixel tiles (3x3: 4 x 16 pixels, 1x1: 64 flat pixels, per image of a group): a split
 * without tiles writes a zero slab and zero bias partials.
 * Alignment (checked): the tile fills move 16 bytes per lane, so every operand's nch and pix_stride are multiples of 4 and
 * its ptr and batch_stride multiples of 16 bytes (4 floats); `zeros` is 16-byte aligned.  A BMC_SRC_TABLE operand's image
 * pointers must be 16-byte aligned too; they live in device memory and are NOT checked. */
typedef struct bmc_pgemm_args {
    bmc_src_t a;                /* nch = M */
    int nsrc;
    bmc_src_t src[BMC_MAX_SRC]; /* sum nch = N */
    int B, H, W, taps;
    int batch_per_group;
    float* slabs;
    int nsplit;
    const float* zeros;         /* >= 64 bytes of zeros in device memory (source for out-of-image LDS-DMA lanes) */
    float* bias_slabs;          /* optional [nsplit][G][4][Mpad]: column sums of A (the bias gradient of the same conv),
                                   taken from the A tiles the kernel stages anyway; summed by bmc_pgemm_reduce_weight */
    int math;                   /* BMC_MATH_* as for bmc_conv; bf16 modes: v_mfma_f32_32x32x16_bf16 on planes read
                                   with the transposing LDS load */
    int tap_groups;             /* 0 / 1: a workgroup accumulates all taps; 3 (taps = 9, fp32 or bf16 arithmetic): one tap row per
                                   workgroup = three times the workgroups per pixel split, for small images (fewer,
                                   smaller slab writes); same slab layout */
} bmc_pgemm_args_t;
int bmc_pgemm(const bmc_pgemm_args_t* host_args, bmc_stream_t s);
/* How bmc_pgemm deals the 8 waves of a workgroup for an fp32 launch with all taps per workgroup: the number of shares the
 * k-steps (pixel pairs) of each pixel tile are cut into.  1: 4 row blocks x 2 column blocks; 2 (taps = 9, N <= 32): 4 row blocks
 * x 2 shares; 4 (taps = 9, M <= 32): 2 column blocks x 4 shares.  The shares are summed in a fixed order inside the workgroup. */
int bmc_pgemm_wave_map(int taps, int M, int N);
/* slabs -> dW[Cout][Cin][taps] (nn.Conv2d layout) through kmap; beta 0/1 = overwrite/accumulate.  kmap: DEVICE array of N ints,
 * slab column n goes to weight column kmap[n] (< Cin; < 0: the column is dropped); columns no entry names are not written.
 * kmap NULL: column n goes to weight column n, which REQUIRES N <= Cin (checked). */
int bmc_pgemm_reduce_weight(const float* slabs, int nsplit, int G, int taps, int M, int N, const int* kmap,
                            int Cin, float* dw, int accumulate, const float* bias_slabs /* or NULL */,
                            float* db /* [G][M] or NULL */, bmc_stream_t s);
/* the same with one destination per group (HOST arrays of G <= 4 device pointers): weights that ONE grouped launch stacks
 * but that belong to separate parameters (v1 / v2, conv_hp / conv_hn) -- each group's sum goes (=|+=) straight to its own
 * dw[g] [M][Cin][taps] / db[g] [M]. */
int bmc_pgemm_reduce_weight_groups(const float* slabs, int nsplit, int G, int taps, int M, int N, const int* kmap,
                                   int Cin, float* const* dw, int accumulate, const float* bias_slabs, float* const* db,
                                   bmc_stream_t s);
/* slabs -> out[G][M][N] * scale */
int bmc_pgemm_reduce_plain(const float* slabs, int nsplit, int G, int M, int N, float scale,
                           float* out, bmc_stream_t s);

/* ---- weight gradient of a dense 3x3, 128 -> 128 channel convolution through the Winograd transform F(2x2, 3x3) ----
 * The same sum as bmc_pgemm (taps = 9) + bmc_pgemm_reduce_weight for this shape -- F.conv2d's weight / bias gradient at
 * models/submodules.py:25-26,33-34 (the residual blocks: 88 % of the network's 3x3 weight-gradient work) -- with 16 instead
 * of 36 multiplies per 2x2 output tile and channel pair on the fp32 MFMA:
 *   dU[xi][nu] = sum over tiles (A dY A^T)[xi][nu]^T (B^T d B)[xi][nu],  dW = G^T dU G,  db = sum of dY;
 * fp32 throughout, deterministic (partial sums per workgroup, added in a fixed order).
 *   dy, x:   NHWC tensors [B,H,W,128] (nch == pix_stride == 128; batch stride / shift / modulus as everywhere);
 *            dy = gradient of the convolution's output, x = its input
 *   nsplit:  workgroups per position row, 1 .. bmc_wgrad_wino_nsplit(B, H, W) (which returns the count that fills the chip)
 *   part:    workspace of nsplit * 16 * 128 * 128 floats;  bias_part: NULL or nsplit * 128 floats
 * bmc_wgrad_wino_reduce:  dw[co][k0 + ci][3][3] (=|+=) the gradient, dw = a [128][ldw][3][3] weight tensor of which the launch's
 * input channels are columns [k0, k0 + 128);  db[128] (=|+=) the bias gradient (bias_part and db go together). */
int bmc_wgrad_wino_nsplit(int B, int H, int W);
int bmc_wgrad_wino(const bmc_src_t* dy, const bmc_src_t* x, int B, int H, int W, int nsplit, float* part, float* bias_part,
                   bmc_stream_t s);
int bmc_wgrad_wino_reduce(const float* part, int nsplit, float* dw, int ldw, int k0, int accumulate, const float* bias_part,
                          float* db, bmc_stream_t s);
/* The same sum over SEVERAL (dy, x) operand pairs in one launch -- the uses of one weight by the weight-sharing blocks of a
 * window (models/BMCNet.py:19-32: `para_reschunk` holds ONE ParallelBlk n_b times), which autograd would add one by one:
 * dy[i], x[i] with batches[i] images each, i < nseg <= 8; nsplit <= bmc_wgrad_wino_nsplit(sum of batches, H, W); the result
 * goes through bmc_wgrad_wino_reduce as before (one partial-sum set, one reduction instead of nseg). */
int bmc_wgrad_wino_multi(const bmc_src_t* dy, const bmc_src_t* x, const int* batches, int nseg, int H, int W, int nsplit,
                         float* part, float* bias_part, bmc_stream_t s);

/* ---- the same weight gradient through F(4x4, 3x3) (round 5): 36 multiplies per 4x4 output tile and channel pair, i.e. 2.25 per
 * output pixel against 4 -- the transform of bmc_conv's BMC_MATH_FP32_WINO4 forward / data-gradient kernel applied to
 * F.conv2d's weight gradient (models/submodules.py:25-26,33-34).  Same operands, same reduce semantics, same determinism;
 * 3.0e-6 rel-L2 per convolution against float64 (contract 1e-3).
 *   nsplit:  workgroups per output slice, 1 .. bmc_wgrad_wino4_nsplit(B, H, W) (8 slices x nsplit workgroups fill the chip)
 *   part:    workspace of nsplit * 36 * 128 * 128 floats;  bias_part: NULL or nsplit * 128 floats */
int bmc_wgrad_wino4_nsplit(int B, int H, int W);
int bmc_wgrad_wino4(const bmc_src_t* dy, const bmc_src_t* x, int B, int H, int W, int nsplit, float* part, float* bias_part,
                    bmc_stream_t s);
int bmc_wgrad_wino4_reduce(const float* part, int nsplit, float* dw, int ldw, int k0, int accumulate, const float* bias_part,
                           float* db, bmc_stream_t s);

/* table[i] = ptrs[i], i < n <= 256: a device table of per-image base pointers for bmc_src_t's BMC_SRC_TABLE mode, written by a
 * kernel on stream s (the pointers travel in its argument block: no host buffer has to outlive the call). */
int bmc_ptr_table(const unsigned long long* ptrs, int n, unsigned long long* table, bmc_stream_t s);

/* ---- streaming kernels ---------------------------------------------------*/
/* out[i] = sum_{k < groups} in[k*n + i] (fixed order): gradient of an operand shared by several batch groups of a launch */
int bmc_group_sum(const float* in, int groups, long long n, float* out, bmc_stream_t s);
/* column sums over pixels (bias gradients): out[c] (+)= sum_p x[p*pix_stride + c]; ws >= 2048*C floats */
int bmc_colsum(const float* x, long long npix, int pix_stride, int C, float* ws, float* out,
               int accumulate, bmc_stream_t s);
/* ReLU backward: g = y > 0 ? dy : 0 (F.relu at models/BMCNet.py:64-80, submodules.py:33) */
int bmc_relu_bwd(const float* dy, const float* y, float* g, long long n, bmc_stream_t s);
/* LayerNorm2d over channels per pixel: models/submodules.py:127-140 (fwd), :141-154 (bwd).
 * stats = [npix][2] (mean, rstd).  bwd: gx, and dgamma/dbeta (+)= via ws (>= 2*1024*C floats). */
int bmc_layernorm_fwd(const float* x, const float* gamma, const float* beta, long long npix, int C,
                      float eps, float* y, float* stats, bmc_stream_t s);
int bmc_layernorm_bwd(const float* dy, const float* x, const float* stats, const float* gamma,
                      long long npix, int C, float* dx, float* ws, float* dgamma, float* dbeta,
                      int accumulate, bmc_stream_t s);
/* row softmax of [rows][C] (torch.softmax(att, -1), models/submodules.py:72-73) and its backward
 * dA = P * (dP - rowsum(dP*P)) * scale_out */
int bmc_softmax_fwd(const float* a, long long rows, int C, float* p, bmc_stream_t s);
int bmc_softmax_bwd(const float* p, const float* dp, long long rows, int C, float scale_out,
                    float* da, bmc_stream_t s);

/* ---- head / tail of a recurrent window -----------------------------------
 * bmc_pack_inputs: models/BMCNet.py:106-112 -- polarity split + x3 repeat of the
 * two frames into two NHWC tensors of 16 channels each
 * [f1,f1,f1,f2,f2,f2,0...] (p: polarity 0, n: polarity 1).  x is [B,2,T,H,W]
 * with arbitrary element strides (sb,sc,st,sy,sx). */
int bmc_pack_inputs(const float* x, long long sb, long long sc, long long st, long long sy, long long sx,
                    int B, int H, int W, int repeat, float* xin_p, float* xin_n, bmc_stream_t s);
/* HR NCHW [B,C,rH,rW] -> LR NHWC [B,H,W,C*r*r] (pixel_unshuffle, models/submodules.py:80-92;
 * also the backward of the head).  split = S > 1 stores the LR tensor as S batch-stacked channel groups
 * [S*B][H][W][C*r*r/S] (group s of sample b at batch s*B + b): with S = 2 that is [o[:, :s^2]; o[:, s^2:]], the operand
 * layout of the input-fusion convolutions (models/BMCNet.py:63) -- no torch.cat between the two.  */
int bmc_unshuffle_to_nhwc(const float* hr, int B, int C, int H, int W, int r, float* lr, int split, bmc_stream_t s);
/* LR NHWC [B,H,W,C*r*r] -> HR NCHW [B,C,rH,rW] (+ bilinear x r of base[B,C,H,W] given with strides
 * (sb,sc,sy,sx), align_corners=False) -- F.pixel_shuffle + F.interpolate + add, models/BMCNet.py:119;
 * base NULL -> pure shuffle (backward of pixel_unshuffle). */
int bmc_shuffle_to_hr(const float* lr, int B, int C, int H, int W, int r, const float* base,
                      long long sb, long long sc, long long sy, long long sx, float* hr, int split /* as above */,
                      bmc_stream_t s);

/* Head + loss of one window in one pass: pred = pixel_shuffle(x_o, r) + bilinear(base) (models/BMCNet.py:119) written to hr
 * [B,C,rH,rW], and loss[0] = mean((pred - gt)^2) (nn.MSELoss, train.py:233,647) from per-block partial sums
 * (partials: >= 2048 floats of workspace; fixed-order reduction).  gt: [B][C][rH][rW] with batch stride gt_batch_stride. */
int bmc_head_mse_fwd(const float* lr, int B, int C, int H, int W, int r, const float* base, long long sb, long long sc,
                     long long sy, long long sx, const float* gt, long long gt_batch_stride, float* hr, float* partials,
                     float* loss, bmc_stream_t s);
/* Its backward: dlr [B,H,W,C*r*r] = pixel_unshuffle(dpred + (2 gloss[0] / numel) (pred - gt)); dpred NULL = no gradient
 * from the next window, gloss (DEVICE scalar) NULL = no gradient from the loss. */
int bmc_head_mse_bwd(const float* dpred, const float* pred, const float* gt, long long gt_batch_stride, const float* gloss,
                     int B, int C, int H, int W, int r, float* dlr, bmc_stream_t s);

/* ---- fused "centre" chain of the BIE block ----------------------------------
 * forward: centre = clustering(LayerNorm2d(convf(cat[s0, s1])))  -- models/submodules.py:63-64 with LayerNormFunction
 * (:127-140) between the two 1x1 convolutions -- in ONE launch: z and y = LN(z) never reach HBM (the second GEMM takes
 * its pixel operand from the first one's accumulator registers).  Saved for backward: yhat = (z - mean)/sqrt(var + eps)
 * (before the affine) and rstd.  C = channels of s0, s1, yhat, centre: 32, 64 or 128.  All outputs are contiguous
 * [B][H][W][C] (rstd [B][H][W]).
 * wstream: 3C/16 slices of [C][16] floats = bmc_pack_weight(W_f, Kpad = 2C, Coutpad = C) followed by
 * bmc_pack_weight(W_c, Kpad = C, Coutpad = C).
 * Paired launches: where B is even and s0 gives launch batches b and b + B/2 the same image for every b < B/2 (the twin
 * layout: s0 with batch_mod = B/2), the kernel may walk the two batches of a pixel tile together and compute the half of
 * convf they share once -- same arguments, same weight stream, bit-identical outputs.  The host decides per launch (more
 * than one pair per CU, and fewer steps on the fullest CU than unpaired).  BMC_CHAIN_PAIR in the environment, read per
 * launch: 0 = never pair; 1 = pair, or fail the call (outputs untouched, bmc_last_error names the reason) if the launch
 * cannot be paired. */
typedef struct bmc_chain_fwd_args {
    bmc_src_t s0, s1;           /* nch = C each; launch batch b reads them through their batch maps */
    const float* wstream;
    const float* bias_f;        /* [C] convf bias */
    const float* bias_c;        /* [C] clustering bias */
    const float* gamma;         /* [C] LayerNorm2d weight */
    const float* beta;          /* [C] LayerNorm2d bias */
    float eps;
    float* yhat;
    float* rstd;
    float* centre;
    int B, C, H, W;
} bmc_chain_fwd_args_t;
int bmc_chain_fwd(const bmc_chain_fwd_args_t* host_args, bmc_stream_t s);

/* backward of the same chain for the twin layout (2n launch batches; batch bb read s0 at bb % n and s1 at (bb + n) % 2n):
 *   dy = W_c^T dcentre;  dz = rstd * (g - yhat*mean_c(g*yhat) - mean_c(g)), g = dy*gamma  (LayerNormFunction.backward, :141-154);
 *   dz  [2n][H][W][C]  is written for the weight-gradient GEMM of convf;
 *   ds1 [(bb + n) % 2n] = W_f[:, C:]^T dz[bb];
 *   ds0 [b] = ds0_add[b] + W_f[:, :C]^T (dz[b] + dz[b + n])   (dz of both halves summed in registers: one GEMM, ds0 written once).
 * Weight / bias / affine gradients: bmc_pgemm on (dcentre, yhat) and (dz, s0, s1) + bmc_chain_affine_grads.
 * wstream: 5C/16 slices of [C][16]: T(W_c), T(W_c), T1(W_f), T1(W_f), T0(W_f) with
 * T(.) = bmc_pack_weight_t(., nkpad = C) and T0 / T1 the operators of W_f's first / second C input channels. */
typedef struct bmc_chain_bwd_args {
    bmc_src_t dcentre;          /* nch = C, 2n launch batches */
    const float* wstream;
    const float* gamma;
    const float* yhat;          /* [2n][H][W][C] from bmc_chain_fwd */
    const float* rstd;          /* [2n][H][W] */
    float* dz;
    float* ds1;
    float* ds0;
    bmc_src_t ds0_add;          /* ptr NULL -> none */
    int n, C, H, W;
} bmc_chain_bwd_args_t;
int bmc_chain_bwd(const bmc_chain_bwd_args_t* host_args, bmc_stream_t s);
/* G[C][C] = bmc_pgemm(dcentre, yhat) reduced with bmc_pgemm_reduce_weight, dbc[C] its bias column sums ->
 * dwc (=|+=) gamma[ci] G[co][ci] + dbc[co] beta[ci];  dgamma[ci] (=|+=) sum_co W_c[co][ci] G[co][ci];  dbeta (=|+=) W_c^T dbc
 * (accumulate 0 | 1; dwc may alias G); dbc_out, if not NULL, (=|+=) dbc. */
int bmc_chain_affine_grads(const float* G, const float* dbc, const float* Wc, const float* gamma, const float* beta, int C,
                           float* dwc, float* dbc_out, float* dgamma, float* dbeta, int accumulate, bmc_stream_t s);

/* ---- batched products of C x C matrices: the BIE's attention without the value tensor --------------------------------
 * models/submodules.py:63-73 computes v = conv1x1(x) and uses it twice, att = scale * bmm(center, v^T) and
 * out = bmm(softmax(att), v).  Both are linear in v = W_v x + b_v, so with G0 = center^T x and s = the column sums of center
 * (one bmc_pgemm launch with bias slabs on x instead of v)
 *     att = scale * (G0 W_v^T + s b_v^T),     out = (P W_v) x + P b_v
 * and v is never formed (bmc_hip/bie.py); the backward likewise needs only C x C matrices.  This entry point evaluates
 * those products for all samples in one launch:
 *     C[b][i][j]  (=|+=) alpha * ( sum_t sum_k A_t[b][i][k] B_t[b][k][j]  +  u[b][i] v[b][j] )
 *     vec[b][i]   (=|+=) alpha *   sum_t sum_k A_t[b][i][k] w_t[b][k]
 * for b < nbatch, i < M, j < N, k < K; t < nterms (1 or 2).  Every operand X of batch b (weight group g = b / batch_per_group)
 * starts at X.ptr + b * X_sb + g * X_sg (floats) and is indexed with its own row / column strides: transposed and per-group
 * operands, and results written into a column range of a wider matrix, need no copies.  u / v (together) and vec_out (with a w
 * in every term) are optional; c may be NULL when only vec_out is wanted.  fp32 FMAs in a fixed order. */
typedef struct {
    const float* a; long long a_sb, a_sg; int a_si, a_sk;   /* A[b][i][k] */
    const float* b; long long b_sb, b_sg; int b_sk, b_sj;   /* B[b][k][j] */
    const float* w; long long w_sb, w_sg; int w_sk;         /* optional w[b][k] */
} bmc_mm_term_t;
typedef struct {
    int nterms;
    bmc_mm_term_t t[2];
    int nbatch, batch_per_group;
    int M, N, K;
    float alpha;
    const float* u; long long u_sb, u_sg;                   /* optional u[b][i] (unit stride) */
    const float* v; long long v_sb, v_sg;                   /*          v[b][j] (unit stride) */
    float* c; long long c_sb, c_sg; int c_si, c_sj;         /* C[b][i][j] */
    float* vec_out; long long vo_sb, vo_sg;                 /* vec[b][i] (unit stride) */
    int accumulate;
} bmc_small_mm_args_t;
int bmc_small_mm(const bmc_small_mm_args_t* host_args, bmc_stream_t s);

/* ---- loss-side resize ------------------------------------------------------
 * F.interpolate(prediction, size=gt.size()[-2:], mode='bicubic', align_corners=False): train.py:227-231,
 * infer_BMCNet.py:77-78 (taken when scale * round(sensor / scale) != sensor, dataloader/h5dataset.py:88-100; EventZoom:
 * 124x224 -> 124x222).  x: `planes` contiguous [H][W] planes (NCHW with planes = B*C) -> y [planes][Ho][Wo].
 * ATen semantics (A = -0.75, source coordinate fma(in/out, dst + 0.5, -0.5), clamped tap indices).  bwd is the transposed
 * operator as a gather: gx[planes][H][W] is OVERWRITTEN, deterministic. */
int bmc_bicubic_resize_fwd(const float* x, long long planes, int H, int W, int Ho, int Wo, float* y, bmc_stream_t s);
int bmc_bicubic_resize_bwd(const float* gy, long long planes, int H, int W, int Ho, int Wo, float* gx, bmc_stream_t s);

/* Head + loss of one window whose ground truth gt [B][C][gh][gw] (contiguous planes, batch stride gt_batch_stride) is NOT of
 * the prediction's size -- head, the resize above and nn.MSELoss (train.py:227-233, _valid :502-506) without the resized
 * prediction or the loss gradient ever reaching memory.  xo [B,H,W,C*r*r], base with strides (sb,sc,sy,sx): as bmc_head_mse_fwd.
 *   pred [B,C,rH,rW]   = pixel_shuffle(xo, r) + bilinear(base): bit for bit what bmc_shuffle_to_hr writes for the same operands
 *                        (it recurs into the next window and must not depend on the loss path); one writer per element.
 *   diff [B,C,gh,gw]   = bicubic(pred -> gh x gw) - gt, taps and summation order of bmc_bicubic_resize_fwd (the four taps of a
 *                        row, then the rows; clamped taps); what the backward reads.  NULL = forward only: nothing is stored.
 *   loss[0]            = sum diff^2 / (B*C*gh*gw) from per-block partial sums (partials: >= 2048 floats of workspace) added in
 *                        a fixed order: deterministic, no atomics.
 * Any gh, gw >= 1.  Null xo / base / gt / pred / partials / loss or a non-positive size: refused before any launch. */
int bmc_head_resize_mse_fwd(const float* xo, int B, int C, int H, int W, int r, const float* base, long long sb, long long sc,
                            long long sy, long long sx, const float* gt, long long gt_batch_stride, int gh, int gw, float* pred,
                            float* diff, float* partials, float* loss, bmc_stream_t s);
/* Its backward: dlr [B,H,W,C*r*r] = pixel_unshuffle(dpred + (2 gloss[0] / (B*C*gh*gw)) R^T diff), R^T = the transposed resize
 * as a gather in bmc_bicubic_resize_bwd's order (deterministic, no atomics).  dpred NULL = no gradient from the next window;
 * gloss (DEVICE scalar) NULL = no gradient from the loss: a pure permutation of dpred, diff is not read.  At least one of the
 * two; diff is required with gloss. */
int bmc_head_resize_mse_bwd(const float* dpred, const float* diff, const float* gloss, int B, int C, int H, int W, int r,
                            int gh, int gw, float* dlr, bmc_stream_t s);

/* The same head with a robust loss (L1, Huber, Charbonnier) in the squared one's place: include/bmc_hip_losses.h. */

/* ---- multi-stream inference: recording slots (bmcnet-esr_amd/infer.py::MultiStreamSR) ------------------------------
 * S <= BMC_MAX_SLOTS independent recordings run through one batched forward pass, recording r in slot s of the batch.  The
 * reference runs one recording at a time at batch 1 (infer_BMCNet.py:248-295 around the loop body :44-86).  Each call below is
 * ONE launch for all S slots; `table` is a DEVICE array of S bmc_slot_t that the host refreshes before each window.
 * Feature states: nfeat tensors (h, h_p, h_n for BMCNet; h for BMCNet_plain) of feat_n = n_c*H*W values per slot, NHWC per
 * slot, laid out [nfeat][S][feat_n] (the model's channels-last [S,n_c,H,W] views, adjacent in one buffer).  The pool holds them
 * in fp32 or bf16 (pool_bf16); the previous prediction [S][pred_n] (pred_n = 2*sH*sW) is always fp32.
 *
 * Self-ensemble (MultiStreamSR(self_ensemble=K)): K adjacent slots carry one recording in K orientations and their predictions
 * are merged into one.  It is table data only -- bits of bmc_slot_t.flags above BMC_SLOT_RESET and the entry's pad_ word; an
 * entry with those bits clear and pad_ == 0 behaves byte for byte as before.
 *   flags bits 2..4: the slot's orientation code o; bit 2 horizontal (h), bit 3 vertical (v), bit 4 polarity (p) -- the order
 *     of bmc_seq_sample_t.flips bits 0..2.  It acts on a finished two-channel image,
 *         O_o(img)[c][y][x] = img[c ^ p][v ? H-1-y : y][h ? W-1-x : x],
 *     an involution; whatever the encoder put into an image (its out-of-range pixel included) moves with the image.
 *   flags bits 8..11: the group size K in {2, 4, 8} at the LEADER of a group, the first of the slots s .. s+K-1 (0, or any
 *     other value: no group).  The caller guarantees that these slots exist, are active and are reset together, that no group
 *     overlaps another, and that the leader's own code is 0: its row is merged as it stands (a lane can overwrite only what it
 *     alone reads).  pad_ at a leader: the prediction's row length sW, with sH = pred_n / (2 sW) (a pad_ <= 0 or one that does
 *     not divide pred_n / 2, or s + K > S: no group); 0 in every other entry.
 *   bmc_slot_stage: an active slot's input is x[s][c][t] = O_o(frames[t])[c]; state and previous prediction as without a code:
 *     every member keeps its own recurrence, in its own orientation.
 *   bmc_slot_commit, at a leader s, after every slot's state and pred_src[s] -> pred_pool[s] copy (the leader's too: its
 *     recurrence continues from its OWN prediction): for every element (c, row, x) of [2][sH][sW], in float32, each operation
 *     rounded on its own and the members taken in slot order,
 *         acc = pred_src[s][c][row][x];  acc = acc + O_{o_j}(pred_src[s+j])[c][row][x]  (j = 1 .. K-1, o_j from entry s+j);
 *         merged = acc * (1.0f / K)                                                       (exact: K is a power of two)
 *     and merged is written to pred_src[s] -- the leader's row of the model's output, IN PLACE -- and to the leader's `keep` if
 *     set.  The lane that owns an element of the leader's row reads it, stores it to pred_pool and only then overwrites it;
 *     member rows are only read; no atomics, no workgroup waits for another: deterministic.  Rows with sW % 4 == 0 take 16-byte
 *     accesses, other rows element loads, with the same bits.  The kernels that run after it (bmc_slot_metrics, bmc_slot_emit*,
 *     bmc_slot_render, bmc_slot_voxel) read pred[s] and skip a slot whose own entry is NULL: with NULL entries for the
 *     members, the leader's entries see the merged prediction. */
#define BMC_MAX_SLOTS 256
#define BMC_SLOT_ACTIVE 1   /* the slot carries a recording this window */
#define BMC_SLOT_RESET 2    /* ... whose first window this is: its state is read as exact zeros (infer_BMCNet.py:55-60) */
typedef struct bmc_slot {
    const float* frames;    /* first frame of the window: [seqn][2][H][W] contiguous (frames[i:i+seqn] of a [L,2,H,W] recording) */
    const float* gt;        /* the window's ground truth [2][gh][gw] (gt of window i = frame i+1, infer_BMCNet.py:49) */
    float* keep;            /* NULL, or where bmc_slot_commit copies the slot's prediction [2][sH][sW] */
    double* result;         /* NULL, or where bmc_slot_metrics writes nparts x {esr_sse, bicubic_sse} partial sums */
    int flags;              /* BMC_SLOT_ACTIVE | BMC_SLOT_RESET; 0 (or frames NULL): an empty slot; bits 2..4, 8..11: self-ensemble */
    int pad_;               /* 0; at the leader of an ensemble group: the prediction's row length sW */
} bmc_slot_t;

/* Before the forward pass (replaces the per-recording input_stack / init_h / init_o tensors of infer_BMCNet.py:51,55-60):
 * x[s] [2][seqn][H][W] = the window of slot s transposed (zeros for an empty slot); feat [nfeat][S][feat_n] fp32 = the pool's
 * state (a bf16 pool widened exactly), exact zeros for a RESET or empty slot -- feat == feat_pool (fp32 pool) loads in place;
 * pred [S][pred_n], read by the model in place, is zeroed for RESET / empty slots. */
int bmc_slot_stage(const bmc_slot_t* table, int S, int seqn, int H, int W, float* x, const void* feat_pool, int pool_bf16,
                   float* feat, int nfeat, long long feat_n, float* pred, long long pred_n, bmc_stream_t s);
/* After the forward pass (the carried h, hp, hn, prediction of infer_BMCNet.py:62-63), active slots only: feat_src = HOST
 * array of nfeat device pointers, each [S][feat_n] fp32 (the model's new states) -> the pool (bf16: round to nearest-even,
 * bit-identical to tensor.to(torch.bfloat16)); pred_src [S][pred_n] -> pred_pool and, where the slot's `keep` is set, there.
 * pred_src is written only at the leader of an ensemble group (above): its row becomes the group's merged prediction. */
int bmc_slot_commit(const bmc_slot_t* table, int S, const float* const* feat_src, int nfeat, long long feat_n, void* feat_pool,
                    int pool_bf16, float* pred_src, float* pred_pool, long long pred_n, bmc_stream_t s);
/* The metrics of infer_BMCNet.py:76-85 as sums of squares, per active slot with a `result`, split into nparts
 * (1 .. BMC_SLOT_MAX_PARTS) partial sums over fixed element sets (element i of [2][gh][gw] in part (i / 1024) % nparts):
 * result[2p] = part p of sum (bicubic(pred[s] -> gh x gw) - gt)^2 (no resize when sH x sW == gh x gw), result[2p+1] = part p
 * of sum (bicubic(frame 1 of the window -> gh x gw) - gt)^2.  ATen's bicubic taps (as bmc_bicubic_resize_fwd); no HR
 * temporary; fixed-order reductions in double, no atomics: the caller adds the parts in a fixed order -- bit-reproducible,
 * independent of the other slots. */
#define BMC_SLOT_MAX_PARTS 64
int bmc_slot_metrics(const bmc_slot_t* table, int S, const float* pred, int sH, int sW, int H, int W, int gh, int gw,
                     int nparts, bmc_stream_t s);

/* Event-backed slots (MultiStreamSR.open_events): the recording stays on the GPU as raw dataset columns (xs / ys int16, ps
 * float64, generate_dataset/tools/event_packagers.py:128-156) and the window's count images are encoded on the fly into
 * per-slot scratch that the slot's bmc_slot_t entry points at (frames = lr_scratch[s], gt = gt_scratch[s]) -- replaces
 * H5Dataset.__getitem__ (dataloader/h5dataset.py:261-316) for the windows that compute_k_indices / get_gt_event_indices_num
 * (:197-215, :362-390) cut.  A second DEVICE table of S entries, parallel to the slot table; lr_xs NULL: the slot has no event
 * entry (empty, or frame-backed).  Every range [first, end) must lie inside its columns: the kernel trusts the table, the
 * host validates the ranges when a recording is opened. */
#define BMC_SLOT_MAX_SEQN 8
typedef struct bmc_slot_events {
    const short* lr_xs;     /* LR columns of the slot's recording */
    const short* lr_ys;
    const double* lr_ps;
    const short* gt_xs;     /* HR (ground-truth) columns */
    const short* gt_ys;
    const double* gt_ps;
    long long gt_range[2];                      /* events [first, end) of the window's ground-truth frame (frame 1 of the window) */
    long long lr_range[BMC_SLOT_MAX_SEQN][2];   /* events [first, end) of the window's LR frames 0 .. seqn-1 (they may overlap) */
} bmc_slot_events_t;
/* ONE launch for all slots with an event entry, before bmc_slot_stage: lr_scratch [S][seqn][2][H][W] and gt_scratch
 * [S][2][gh][gw] <- the count images of the ranges, bit-identical to bmc_encode_raw_events without flips (out-of-range quirk
 * included) for integer-valued polarities (+-1 in the datasets; a weight p*p is counted as an integer).  Slots without an
 * entry are not touched.  A workgroup owns a band of rows of one frame: zeroed in LDS, counted with integer LDS atomics,
 * stored once (the store is the zero fill) -- no global float atomics, no memset, order independent and run-to-run identical.
 * W, gw <= 7680; 2 <= seqn <= BMC_SLOT_MAX_SEQN. */
int bmc_slot_encode(const bmc_slot_events_t* table, int S, int seqn, int H, int W, int gh, int gw, float* lr_scratch,
                    float* gt_scratch, bmc_stream_t s);

/* ---- sequence encoder for training ----------------------------------------
 * The training counterpart of the event-backed slots (event_dataset.EventTrainSet.batch): recordings stay on the GPU as raw
 * dataset columns and ONE launch per batch encodes every LR and HR count image of B sequences of L items into the collate
 * layout inp_cnt [B][L][2][H][W], gt_cnt [B][L][2][gh][gw] -- what SequenceDataset.__getitem__ (dataloader/h5dataset.py:666-700)
 * has H5Dataset.__getitem__ (:261-316) do per item in the loader's workers.  A DEVICE table of B entries:
 *   LR item t, not paused: the count image bmc_encode_raw_events gives for events [first, end) of lr_range[t] with `flips`
 *     (augment_event :559-578: the flip is applied to the int16 coordinate and the polarity BEFORE the range test, so the
 *     out-of-range quirk applies to the flipped values: an out-of-range negative adds 1 at [H-1][0] of channel 1, an
 *     out-of-range positive counts nowhere), plus the sample's n_noise noise events, NOT flipped (:281-285: the noise is
 *     concatenated after augment_event) and under the same range rule (add_noise_event :623-634 can give x == W or y == H:
 *     out of range).
 *   LR item t, paused (bit t of `paused`): all +0.0 -- no events, no noise (:304-306).
 *   HR item t: gt_range[t] encoded with the same `flips` at (gh, gw), paused or not, never with noise.
 * Polarities are -1 / 0 / +1 and counters are integers (a weight p*p is counted as an integer); below 2^24 events per pixel
 * the result is the float32 sum of the reference.  The scheme is bmc_slot_encode's: a workgroup owns a band of rows of one
 * frame, at most 60 KB of LDS counters, integer LDS atomics, stored once (the store is the zero fill) -- no global atomics, no
 * memset, order independent and run-to-run identical.  Limits the CALLER checks and the kernel trusts: every range inside its
 * columns, first <= end; checked here: 2 <= L <= BMC_SEQ_MAX_ITEMS, W, gw <= 7680, 1 <= B <= 65535.
 * Bit 3 of `flips` (transpose) means something to bmc_seq_encode_crop only: bmc_seq_encode has one output size per launch, which
 * a transposed frame does not have, and ignores the bit -- flips | 8 gives the bytes of flips & 7. */
#define BMC_SEQ_MAX_ITEMS 32
typedef struct bmc_seq_sample {           /* one sequence of the batch */
    const short* lr_xs;     /* its recording's LR columns */
    const short* lr_ys;
    const double* lr_ps;
    const short* gt_xs;     /* HR (ground-truth) columns */
    const short* gt_ys;
    const double* gt_ps;
    const short* noise_xs;  /* n_noise noise events; NULL / 0: none */
    const short* noise_ys;
    const signed char* noise_ps;
    int n_noise;
    unsigned flips;         /* bit0 horizontal, bit1 vertical, bit2 polarity (as bmc_encode_raw_events); bit3 transpose:
                               bmc_seq_encode_crop only (below), ignored by bmc_seq_encode; higher bits are ignored */
    unsigned paused;        /* bit t: item t is a paused frame */
    long long lr_range[BMC_SEQ_MAX_ITEMS][2];   /* events [first, end) of LR item t; ranges may overlap */
    long long gt_range[BMC_SEQ_MAX_ITEMS][2];
} bmc_seq_sample_t;
int bmc_seq_encode(const bmc_seq_sample_t* table, int B, int L, int H, int W, int gh, int gw, float* inp_cnt, float* gt_cnt,
                   bmc_stream_t s);
/* Patch training (event_dataset.EventTrainSet(crop=...)): the same table, and parallel to it a DEVICE table of B crops; ONE
 * launch writes one patch per sample, inp_cnt [B][L][2][h][w] and gt_cnt [B][L][2][scale*h][scale*w], so that recordings of
 * different sensor sizes share a batch.  For every sample b the outputs are, bit for bit, the slices
 *   full_inp[b][:, :, top:top+h, left:left+w]      full_gt[b][:, :, scale*top:scale*(top+h), scale*left:scale*(left+w)]
 * of what bmc_seq_encode writes for the same table entry at the sample's own (H, W, gh, gw): the flips act on the full frame,
 * before the range test; an out-of-range negative adds 1 at [fh-1][0] of channel 1 of the FULL frame and is in the patch only
 * when the patch covers that pixel; noise events are unflipped and ranged against the sample's own (H, W); a paused LR item is
 * all +0.0; HR items never get noise; zeros are +0.0.  The scheme is bmc_seq_encode's on the patch: a workgroup owns a band of
 * min(15360 / (2 * patch width), patch height) rows of one patch frame, zeroed in LDS, counted with integer LDS atomics, stored
 * once -- no global atomics, no memset, order independent and run-to-run identical; a band reads xs / ps of every event only when
 * it holds the full frame's [fh-1][0] (left == 0 and the band covers row fh-1).  Checked here: 1 <= B <= 65535, 2 <= L <=
 * BMC_SEQ_MAX_ITEMS, scale >= 1, h, w >= 1, scale * w <= 7680 (the limit is the patch's, not the recording's).  The CALLER
 * checks and the kernel trusts: every range inside its columns, and the crop inside the frames: top, left >= 0, top + h <= H,
 * left + w <= W, scale * (top + h) <= gh, scale * (left + w) <= gw.
 * Transpose (bit 3 of the sample's `flips`; with the two flips it gives all 8 orientations of a patch -- rot90 is one flip followed
 * by the transpose).  Let F_lr[b] [L][2][H][W] and F_gt[b] [L][2][gh][gw] be what bmc_seq_encode writes for the same entry with
 * flips & 7 at the sample's own sizes: flips before the range test, the out-of-range quirk, the unflipped noise and the paused
 * items included.  Bit 3 clear: the slices above, as ever.  Bit 3 set, s = scale:
 *   inp_cnt[b] = F_lr[b].transpose(-1,-2)[..., top:top+h, left:left+w]
 *   gt_cnt[b]  = F_gt[b].transpose(-1,-2)[..., s*top:s*(top+h), s*left:s*(left+w)]
 * The transpose acts on the finished image and carries the noise and the quirk pixel with it: the full frame's [fh-1][0] of
 * channel 1 is [0][fh-1] of the transposed frame and is in the patch only when top == 0 and left <= fh-1 < left + w (scaled
 * likewise for HR).  top and left are rows / columns of the TRANSPOSED frame, and the caller checks top + h <= W, left + w <= H,
 * s * (top + h) <= gw, s * (left + w) <= gh.  So the transposed h x w patch at (top, left) is the transpose of the untransposed
 * w x h patch at (left, top).  Samples with and without the bit share the launch (the choice is uniform per workgroup); the scheme
 * is unchanged: a band of a transposed sample tests the coordinate that becomes its row first -- xs, after its flip against fw --
 * and reads ys / ps only of events that can land in it, except the band that holds [0][fh-1], which reads everything. */
typedef struct bmc_seq_crop {   /* one per sample, parallel to the bmc_seq_sample_t table */
    int H, W, gh, gw;           /* the sample's OWN full frame sizes (flips and the out-of-range rule use these), never swapped */
    int top, left;              /* patch origin in LR IMAGE rows / columns (row 0 = sensor y = H-1); of a transposed sample: in
                                   the transposed image (row 0 = sensor x = 0, column 0 = sensor y = H-1) */
} bmc_seq_crop_t;
int bmc_seq_encode_crop(const bmc_seq_sample_t* table, const bmc_seq_crop_t* crops, int B, int L, int h, int w, int scale,
                        float* inp_cnt, float* gt_cnt, bmc_stream_t s);

/* Event OUTPUT of the slots (MultiStreamSR(emit_events=True)): the window's prediction leaves the session as an event list
 * appended to the recording's own output columns -- the rounded count image the reference renders (infer_BMCNet.py:94:
 * esr_cnt[0].cpu().round()), clamped, as the stream whose encoding gives that image back.  Per element v of pred[s]
 * [2][sH][sW], visited in flat order:  q = v > 0 ? min(rint(v), max_count) : 0  (round-half-to-even on the fp32 value; NaN ->
 * 0, +inf -> max_count); element (c, row, x) contributes q consecutive events xs = x, ys = sH-1-row, ps = c == 0 ? +1 : -1
 * (the inverse of bmc_slot_encode / bmc_encode_raw_events without flips: encoding the emitted events at (sH, sW) gives q).
 * A third DEVICE table of S entries, parallel to the slot table; xs NULL (or an inactive slot): the slot emits nothing.
 * The event at global position g of the recording is stored at xs[g], ys[g], ps[g] when g < capacity and dropped otherwise;
 * *index_out = *index_in + the window's event count ALWAYS (the true running count, also past the capacity).  index_in and
 * index_out must be different words (entries i and i+1 of the recording's index table). */
typedef struct bmc_slot_emit {
    short* xs;                  /* output columns of the slot's recording, `capacity` entries each */
    short* ys;
    signed char* ps;
    const long long* index_in;  /* events emitted before this window */
    long long* index_out;       /* ... and after it */
    long long capacity;
} bmc_slot_emit_t;
/* TWO launches for all slots, grid (nparts, S), after the forward pass: a count pass (part p sums q over elements [p*chunk,
 * (p+1)*chunk) of the slot, chunk = ceil(2*sH*sW / nparts) rounded up to 4, into parts[s][p]) and a write pass (part p starts
 * at *index_in + the parts before it, scans its chunk and stores the events at their final positions).  No workgroup waits for
 * another, no atomics; integer counts, the same bytes run after run.  parts: S x nparts words of scratch.  sH, sW <= 32767
 * (int16 coordinates); 1 <= max_count <= 32767; 1 <= nparts <= BMC_SLOT_EMIT_MAX_PARTS and chunk * max_count < 2^32. */
#define BMC_SLOT_EMIT_MAX_PARTS 1024
int bmc_slot_emit(const bmc_slot_t* table, const bmc_slot_emit_t* emit, int S, const float* pred, int sH, int sW, int max_count,
                  int nparts, unsigned* parts, bmc_stream_t s);

/* TIMED event output (MultiStreamSR(emit_events=True, event_times="linear")): the same events, each with a float32 time
 * inside its window, every window stored in time order -- the reference's linear redistribution of a count image
 * (dataloader/encodings.py:367-414, python_event_redistribute_PolarityStack, mode='linear', one time bin) with the sort on
 * the GPU.  Per slot and window, with q, the flat order (c, row, x) and xs / ys / ps exactly as bmc_slot_emit defines them:
 *   Time.   Event j (0 <= j < n) of an element with n = q events has  t = (float)(T0 + (T1 - T0) * j / (n - 1)),  evaluated in
 *           float64 (the product first, then the quotient, then the sum) and rounded ONCE to float32; n = 1 gives (float)T0.
 *           T0 = BMC_EVENT_T0 = 0.01, T1 = BMC_EVENT_T1 = 1.0: linspace(c/bins + 1/(100*bins), (c+1)/bins, n) at bins = 1, c = 0.
 *   Order.  The window's events are ordered by the EXACT rational j / (n - 1) (0 for n = 1), ascending; equal rationals (1/2 =
 *           2/4, every j = 0, every j = n-1) keep the flat emission order of bmc_slot_emit: a stable sort.  (The rounded
 *           float is NOT the key, though it is non-decreasing along the sorted window.)
 *   Limit.  max_count <= BMC_SLOT_EMIT_TIMED_MAX_COUNT = 255: distinct rationals with denominators <= 254 differ by at least
 *           1 / (254 * 253) and there are fewer than 2^16 of them, so their dense rank is an exact 16-bit sort key.
 *           rank_table: DEVICE [256][256] uint16, rank_table[n][j] = the number of distinct fractions p/d (1 <= d <= 254,
 *           0 <= p <= d) smaller than j / (n - 1) (0 for n = 1), for 0 <= j < n; built by the host in integer arithmetic.
 *   Storage. The window occupies [*index_in, *index_out) of the recording's columns, *index_out = *index_in + its event count
 *           ALWAYS; the event at global position g is stored at xs[g], ys[g], ps[g], ts[g] when g < capacity and dropped
 *           otherwise (bmc_slot_emit's rule).  The sort works in `scratch`, which holds window_capacity events per slot: a
 *           window of more events stores NOTHING (its columns keep their bytes) and still advances the index by its true
 *           count -- the caller compares index differences with window_capacity.
 *   Determinism. Integer keys and counts; no workgroup waits for another; no atomics on global memory; grids fixed by the
 *           arguments, the live sizes are read from device memory: the same bytes run after run, capturable in a graph.
 * The device table entry: the fields of bmc_slot_emit_t, then ts. */
#define BMC_EVENT_T0 0.01
#define BMC_EVENT_T1 1.0
#define BMC_SLOT_EMIT_TIMED_MAX_COUNT 255
#define BMC_SLOT_EMIT_TIMED_BLOCK 4096                  /* records per workgroup of the second digit pass */
#define BMC_SLOT_EMIT_TIMED_MAX_WINDOW (1ll << 28)      /* window_capacity limit */
typedef struct bmc_slot_emit_timed {
    short* xs;                  /* output columns of the slot's recording, `capacity` entries each */
    short* ys;
    signed char* ps;
    const long long* index_in;  /* events emitted before this window */
    long long* index_out;       /* ... and after it */
    long long capacity;
    float* ts;                  /* the time column, parallel to xs / ys / ps */
} bmc_slot_emit_timed_t;
/* SIX launches for all slots (csrc/slot_emit_timed.hip): a stable least-significant-digit radix sort on the 16-bit rank in
 * two 8-bit passes.  count (nparts, S): part totals and low-digit histograms; scan (S): the slot's total, *index_out, exclusive
 * offsets over (digit, part); expand (nparts, S): every event's record (flat element index, rank, j, n) to its position by low
 * digit in scratch; histogram (blocks, S): high digits of blocks of BMC_SLOT_EMIT_TIMED_BLOCK records; scan (S); scatter
 * (blocks, S): xs / ys / ps / ts to *index_in + the position by high digit.  blocks = ceil(window_capacity / BLOCK).
 * parts: S x nparts words; scratch: bmc_slot_emit_timed_scratch_bytes(S, nparts, window_capacity) bytes, 8-byte aligned (-1 for
 * arguments out of range).  Limits of bmc_slot_emit, and max_count <= 255, 1 <= window_capacity <= 2^28. */
long long bmc_slot_emit_timed_scratch_bytes(int S, int nparts, long long window_capacity);
int bmc_slot_emit_timed(const bmc_slot_t* table, const bmc_slot_emit_timed_t* emit, int S, const float* pred, int sH, int sW,
                        int max_count, int nparts, unsigned* parts, const unsigned short* rank_table, void* scratch,
                        long long window_capacity, bmc_stream_t s);

/* CLOCKED event output (MultiStreamSR.open / open_events with spans= or lr_ts=): the timed stream with float64 times on the
 * RECORDING'S OWN CLOCK.  The caller supplies, per slot and window, the time span [t_first, t_last] of the item the window
 * predicts (sensor microseconds, epoch seconds, ...: float32 cannot hold such a time base).  Counts, the event set, xs / ys /
 * ps, the order (the exact rational j / (n - 1), ties in flat emission order), the storage rule, both capacity rules and the
 * determinism are EXACTLY those of the timed output above; only the time column differs:
 *   Time.   For event j of an element's n events let g = gcd(j, n - 1).  In float64,
 *             tau = T0 + (T1 - T0) * (j / g) / ((n - 1) / g)   (the product first, then the quotient, then the sum; tau = T0
 *                                                               for n = 1; j / g and (n - 1) / g are exact integers),
 *             t   = t_first + tau * (t_last - t_first)         (a float64 multiply and a float64 add, each rounded on its own:
 *                                                               never a fused multiply-add),
 *           and t is stored as float64.  The REDUCED fraction matters: the unreduced float64 expression gives values one ulp
 *           apart for equal rationals (925 of the 19 693 distinct rationals with n <= 255), which float32 rounding hides but
 *           a float64 column would show as a decrease inside a run of ties.  With it every rational has one tau, tau is
 *           strictly increasing in the rational, (float)tau equals the timed output's float32 time for every (j, n), and t is
 *           non-decreasing along every sorted window for any t_last >= t_first.
 *           This inverts the normalisation of BaseDataset.event_formatting (dataloader/base_dataset.py:30), ts_norm =
 *           (ts - ts[0]) / (ts[-1] - ts[0] + 1e-6), WITHOUT its 1e-6: tau = T1 = 1 lands on t_last exactly.
 * A fourth DEVICE table of S entries, parallel to the other three, refreshed per window like them (so the call works inside a
 * captured graph).  ts NULL: the slot is not clocked and gets the timed output's float32 column (its emit entry's ts) -- one
 * launch sequence serves a session of both kinds.  ts non-NULL: the slot's emit entry's float32 ts is not written and may be
 * NULL.  The same SIX launches: only the scatter kernel reads this table. */
typedef struct bmc_slot_clock {
    double t_first;             /* time of the first ... */
    double t_last;              /* ... and of the last event of the item this window predicts; finite, t_last >= t_first */
    double* ts;                 /* NULL, or the recording's float64 time column, `capacity` entries, parallel to xs / ys / ps */
} bmc_slot_clock_t;
/* Arguments, limits and scratch of the timed call, and `clock` (8-byte aligned). */
int bmc_slot_emit_clocked(const bmc_slot_t* table, const bmc_slot_emit_timed_t* emit, const bmc_slot_clock_t* clock, int S,
                          const float* pred, int sH, int sW, int max_count, int nparts, unsigned* parts,
                          const unsigned short* rank_table, void* scratch, long long window_capacity, bmc_stream_t s);

/* ---- hot-pixel filter of event-backed slots (MultiStreamSR(hot_filter=dict(max_px, min_obvs, max_rate))) -----------------
 * The reference carries the filter as dataset.hot_filter.{enabled,max_px,min_obvs,max_rate} (infer_BMCNet.py:178), the state
 * hot_events / hot_idx (dataloader/h5dataset.py:155-156), create_hot_mask (:528-548) and get_hot_event_mask
 * (dataloader/encodings.py:349-364); it computes the mask but never applies it (__getitem__ does not call create_hot_mask), so
 * rules 1-3 restate the reference and rules 4-5 are this project's statement of how the mask meets the count image.
 * THE CONTRACT.  One recording, LR items 0 .. L-1 (lr_index), sensor (H, W), parameters max_px >= 0, min_obvs >= 0 (integers)
 * and a finite max_rate:
 *   1. Observation.  obs_j[y][x] = events_to_mask of item j's LR events (bmc_events_to_mask, oracle.events_to_mask_np): row =
 *      the event's y (no vertical flip), value = |p| of the LAST event in column order that maps to the pixel; an out-of-range
 *      event maps to (0, 0) with weight 0 (it can clear [0][0]).  Polarities are -1 / 0 / +1, so obs_j is 0 or 1.
 *   2. Running count.  count_j = obs_0 + ... + obs_j (integers), idx_j = j + 1: every item is seen once, in item order, however
 *      many windows it appears in.
 *   3. Mask.  mask_j = get_hot_event_mask(float32(count_j) / float32(idx_j), idx_j, max_px, min_obvs, max_rate), 1 = keep.
 *      On the integers: cmin = the smallest c in [0, idx] with float32(c) / float32(idx) > float32(max_rate) (idx + 1 if there
 *      is none; the host evaluates this in float32 and hands the kernel an integer).  If idx > min_obvs, the pixels with count
 *      >= cmin are masked, at most max_px of them, the largest counts first and equal counts in flat row-major order (argmax
 *      returns the first maximum).  For idx < 2^23 distinct counts give distinct float32 rates, so the order by count is the
 *      order by rate; a filtered session refuses L >= 2^23.
 *      max_rate < 0: the reference's loop zeroes the rate it masks, and 0 > max_rate, so it finds that entry again.  Its result:
 *      the pixels with count >= 1 are masked by the rule above and, if fewer than max_px of them exist, ONE more pixel -- the
 *      first maximum of the zeroed image, which is pixel (0, 0).  (Not "every pixel": the loop never leaves that entry.)
 *   4. Filtered frame j = the count image of item j as bmc_slot_encode builds it, with BOTH channels set to exactly 0 at
 *      [H-1-y][x] for every (y, x) with mask_j[y][x] == 0 (so the out-of-range negatives on [H-1][0] of channel 1 go when
 *      sensor pixel (0, 0) is masked).
 *   5. Window i reads filtered frames i .. i+seqn-1, each with its OWN mask_j: a ring of seqn masks per slot, item j at ring
 *      position j % seqn.  The first window of a recording observes items 0 .. seqn-1 in order, every later window item
 *      i+seqn-1.  The ground-truth frame is not filtered; the bicubic baseline of bmc_slot_metrics reads the filtered middle
 *      frame (the scratch it already reads).
 * Consequence: a filtered event-backed recording is bit-identical to open() on the frames rules 1-4 give.
 *
 * A fifth DEVICE table of S entries, parallel to the slot and event tables.  An all-zero entry is the inactive form: a slot that
 * is empty, frame-backed or not filtered -- neither call below touches anything of it. */
typedef struct bmc_slot_hot {
    int* hot_pixels;            /* NULL, or where the number of pixels masked for the window's LAST item is written */
    unsigned char* hot_mask;    /* NULL, or [H][W] (sensor coordinates, 1 = kept): the mask of the window's last item */
    int first_item;             /* item index i of the window's frame 0: frame t is item i + t, ring position (i + t) % seqn */
    int new_from;               /* the first newly observed frame: 0 at a reset (the counts restart from zero), else seqn - 1 */
    int active;                 /* 0: the slot is not filtered */
    int pad_;
    int cmin[BMC_SLOT_MAX_SEQN];/* per frame t >= new_from: rule 3's cmin for its item (1 with negative_rate); <= 0: idx <= min_obvs,
                                   the item masks nothing */
} bmc_slot_hot_t;
/* ONE launch for all slots, before the encode launch (csrc/slot_hot.hip): for each newly observed frame of each active slot, in
 * order: the last-writer observation (integer atomicMax over event indices in ws), counts += obs, the selection of rule 3, the
 * item's mask into ring[s][(first_item + t) % seqn].  `events` is the window's event table (columns and lr_range).
 * counts [S][H][W] int32, ring [S][seqn][H][W] uint8 (1 = keep), ws [S][H][W] int32 of workspace.  negative_rate: max_rate < 0.
 * One workgroup per slot, no workgroup waits for another, integers only, global accesses only; the grid is fixed by S and the
 * live values are read from device memory: the same bytes run after run, capturable in a graph.  Every LR item range must be
 * shorter than 2^31 events. */
int bmc_slot_hot_update(const bmc_slot_hot_t* hot, const bmc_slot_events_t* events, int S, int seqn, int H, int W, int max_px,
                        int negative_rate, int* counts, unsigned char* ring, int* ws, bmc_stream_t s);
/* bmc_slot_encode for a filtered session: an LR band of a slot with an active hot entry is multiplied by its item's mask when it
 * is stored (rule 4: both channels, flipped row); ground-truth bands and slots without an active entry are stored as
 * bmc_slot_encode stores them.  ONE launch, the same grid. */
int bmc_slot_encode_filtered(const bmc_slot_events_t* table, const bmc_slot_hot_t* hot, const unsigned char* ring, int S, int seqn,
                             int H, int W, int gh, int gw, float* lr_scratch, float* gt_scratch, bmc_stream_t s);
/* get_hot_event_mask (dataloader/encodings.py:349-364) on a float32 [H][W] image: the same selection code on a monotone
 * unsigned image of the values (-0.0 orders as +0.0).  mask [H][W] float32 <- 1 / 0; the selected entries of event_rate are
 * zeroed IN PLACE as the reference does.  active = (idx > min_obvs).  Any NaN: nothing is masked (argmax finds the NaN, which is
 * not > max_rate, and the loop stops).  max_rate < 0: after the positive entries, what is left of max_px goes to ONE entry, the
 * first in flat order that is >= 0 (it becomes +0.0), or, when every entry is negative, the first maximum if it is > max_rate.
 * ws: H*W words.  One workgroup. */
int bmc_hot_pixel_mask(float* event_rate, int H, int W, int active, int max_px, float max_rate, float* mask, unsigned* ws,
                       bmc_stream_t s);

/* ---- event-count images of the slots (MultiStreamSR(render=...)) ---------------------------------------------------------
 * The reference's inference writes four rendered images per window (infer_BMCNet.py:90-97) with
 * event_visualisation.plot_event_cnt (myutils/vis_events/matplotlib_plot_events.py:125-248), called with its defaults
 * (color_scheme="blue_red", use_opencv=False, is_black_background=False, is_norm=True).
 * THE CONTRACT is the uint8 [h][w][3] array that function RETURNS for a float32 count image cnt [2][h][w] (channel 0 positive,
 * 1 negative); the PNG matplotlib then draws from it at 300 dpi is not part of it.  N = h * w:
 *   1. Percentiles.  Per channel c: min_c = np.percentile(cnt[c], 1), max_c = np.percentile(cnt[c], 99), as NumPy 2.x computes
 *      them for a FLOAT32 array (method "linear"): q = float32(1) / float32(100) resp. float32(99) / float32(100); the virtual
 *      index vi = float32(N - 1) * q, ONE float32 product (not float64: np.percentile divides by the array's own float32(100),
 *      and a 0-d float32 array times a Python int stays float32); k = floor(vi), gamma = vi - k (exact), the neighbours are the
 *      order statistics k and k + 1 (both N - 1 when vi >= N - 1, i.e. N = 1) of the sorted channel; the result is NumPy's lerp
 *      in float32, every operation rounded on its own:  d = b - a;  gamma >= 0.5 ?  b - d * (1 - gamma)  :  a + d * gamma.
 *      mx = max_0 > max_1 ? max_0 : max_1.
 *   2. Normalisation.  Per channel: if min_c != mx then v = (v - min_c) / (mx - min_c) in float32 (the division correctly
 *      rounded, no fused multiply-add); otherwise the channel is left AS IT IS (the reference's quirk).  Then clip to [0, 1].
 *   3. Colour.  p, n = the two clipped channels.  p > 0 and (n == 0 or p >= n): (c0, c1, c2) = (1, 1 - p, 1 - p); else n > 0:
 *      (1 - n, 1 - n, 1); else (1, 1, 1).  1 - p is a float32 difference; byte = trunc((double)c * 255.0).  The BGR -> RGB
 *      conversion reverses the triple: out[y][x] = (byte(c2), byte(c1), byte(c0)) -- positive counts come out blue, negative red.
 *   `round` != 0: every value is first rounded half-to-even (rintf), as infer_BMCNet.py:94 rounds the prediction.
 *   A -0.0 is treated as +0.0 (it cannot change a byte).  Non-finite inputs are OUTSIDE the contract: the call is safe for them
 *   and its bytes are unspecified.  Limits: 1 <= h * w <= BMC_SLOT_RENDER_MAX_PIXELS = 2^24 (N - 1 exact in float32).
 * A DEVICE table of S entries, parallel to the slot table: src NULL, dst NULL or an inactive slot: nothing of the slot is read or
 * written.  dst needs no alignment (a 4-byte aligned dst is stored in 32-bit words). */
#define BMC_SLOT_RENDER_MAX_PIXELS (1 << 24)
#define BMC_SLOT_RENDER_MAX_PARTS 1024
typedef struct bmc_slot_render {
    const float* src;           /* the count image [2][h][w] */
    unsigned char* dst;         /* the rendered image [h][w][3] */
} bmc_slot_render_t;
/* TWO launches for all slots (csrc/slot_render.hip).  select, grid (2, S): one workgroup per (channel, slot) finds the four order
 * statistics of rule 1 exactly, by an 8-bit radix select over order-preserving 32-bit keys of the values (four passes over the
 * plane, one 256-bin LDS histogram per tracked rank, integer LDS atomics), and writes (min_c, max_c) to scratch.  colour, grid
 * (nparts, S), 1 <= nparts <= BMC_SLOT_RENDER_MAX_PARTS: rules 2 and 3, four pixels per lane.  scratch: 4 * S floats.  No float
 * atomics, no global atomics, no dependence on other slots, no workgroup waits for another: the same bytes run after run,
 * capturable in a graph. */
int bmc_slot_render(const bmc_slot_t* table, const bmc_slot_render_t* render, int S, int h, int w, int round, int nparts,
                    float* scratch, bmc_stream_t s);

/* ---- voxel grids of the slots' predictions (MultiStreamSR(voxel_bins=B)) ---------------------------------------------------
 * The temporal-bilinear voxel grid of a window's super-resolved events, as the reference's events_to_voxel_torch
 * (dataloader/encodings.py:100-148, temporal_bilinear=True) computes it -- per output pixel, without building the event stream.
 * THE CONTRACT.  Input: a slot's prediction P [2][sH][sW] (float32), bins, max_count (1 <= max_count <= 255).  With q as
 * bmc_slot_emit defines it (q = min(rint(v), max_count) for v > 0, else 0; NaN gives 0), out [bins][sH][sW] (float32) equals, bit
 * for bit, what events_to_voxel_torch(xs, ys, ts, ps, bins, sensor_size=(sH, sW)) returns for the window's TIMED stream: the
 * columns of bmc_slot_emit_timed for the same P and max_count as float32 (xs = x, ys = sH-1-row, ps = +1 for channel 0 and -1
 * for channel 1, ts the times).
 *   1. Empty.  N = the sum of q.  N <= 3: out is all zeros (the reference's len(ts) <= 3; its ts.sum() == 0 cannot occur, every
 *      time is at least 0.01).
 *   2. Window.  Otherwise t_first = float32(0.01) (the stream's first event has j = 0); t_last = float32(1.0) if any q >= 2, else
 *      float32(0.01) (the stream's last event); dt = (t_last - t_first) + 1e-6f; bm1 = float(bins - 1).
 *   3. Events of a pixel.  Output pixel (y, x) reads row = sH-1-y of the prediction: its events are those of q0 = q[0][row][x]
 *      with p = +1 and of q1 = q[1][row][x] with p = -1; event j of n has the timed output's float32 time, (float)(T0 + (T1 - T0)
 *      * j / (n - 1)) evaluated in float64 and rounded once, (float)T0 for n = 1.
 *   4. Order.  The two runs are merged by the EXACT rational j / (n - 1) (0 for n = 1), compared by integer cross-multiplication;
 *      on equal rationals channel 0 comes first -- the order of the timed stream restricted to the pixel.
 *   5. Accumulation.  For every event in that order and every bin b:  tn = ((t - t_first) / dt) * bm1;  w = fmaxf(0, 1 -
 *      fabsf(tn - b));  acc_b = acc_b + p * w -- every operation a float32 operation rounded on its own (no fused multiply-add,
 *      IEEE division), the order of the reference's index_put_(accumulate=True).  out[b][y][x] = acc_b.
 *   ROWS.  out's rows are the SENSOR'S y: they are vertically flipped against the prediction's rows (out[b][y][x] comes from
 *   P[c][sH-1-y][x]), exactly as the reference's function gives for the emitted ys.
 *   The grid is window-normalised: the reference subtracts ts[0] and divides by the span, so a sensor clock does not change it.
 *   Determinism.  No atomics, no workgroup waits for another, the partials are folded in part order by every workgroup: the
 *   same bytes run after run, eager or replayed from a graph; a slot's grid does not depend on its neighbours.
 *   Limits: 1 <= bins <= BMC_SLOT_VOXEL_MAX_BINS = 32; max_count <= 255 (the timed output's limit: the times are defined for
 *   n <= 255); sH, sW <= 32767; 1 <= nparts <= BMC_SLOT_EMIT_MAX_PARTS and chunk * max_count < 2^32 as for bmc_slot_emit.
 * A DEVICE table of S entries, parallel to the slot table.  A slot takes part when it is active, has a prediction (frames) and
 * its entry has a dst; nothing of any other slot is read or written. */
#define BMC_SLOT_VOXEL_MAX_BINS 32
typedef struct bmc_slot_voxel {
    float* dst;                 /* NULL, or the grid [bins][sH][sW] */
} bmc_slot_voxel_t;
/* TWO launches for all slots (csrc/slot_voxel.hip), no memset.  reduce, grid (nparts, S): part p sums q and takes the largest q
 * over elements [p*chunk, (p+1)*chunk) of the slot (chunk as bmc_slot_emit) -> parts[s][0][p], parts[s][1][p].  voxel, grid
 * (nparts, S): every workgroup folds its slot's partials, then owns output pixels [p*pchunk, (p+1)*pchunk), pchunk =
 * ceil(sH*sW / nparts): two loads and `bins` stores per pixel, coalesced along x.  parts: 2 * S * nparts words of scratch. */
int bmc_slot_voxel(const bmc_slot_t* table, const bmc_slot_voxel_t* voxel, int S, const float* pred, int sH, int sW, int max_count,
                   int bins, int nparts, unsigned* parts, bmc_stream_t s);

/* ---- optimizer step (bmcnet-esr_amd/bmc_hip/optim.py::Adam) ----------------------------------------------------------------
 * torch.optim.Adam(amsgrad, weight_decay) as train.py:653 builds it and train.py:237 steps it, for ALL parameters of a group in
 * ONE launch over a DEVICE table of chunks.  A chunk is at most BMC_ADAM_CHUNK = 4096 consecutive elements of ONE tensor (a tensor
 * of n elements gives ceil(n / 4096) chunks; a chunk never spans two tensors); the grid is n_chunks workgroups of 256 lanes.
 * Per element, in float32, every line ONE correctly rounded operation (no fused multiply-add, IEEE square root and division):
 *     g' = g + weight_decay * p        (skipped when weight_decay == 0; g itself is never written)
 *     m  = m + one_minus_beta1 * (g' - m)
 *     v  = v * beta2 + one_minus_beta2 * (g' * g')
 *     vmax = max(vmax, v)              (amsgrad; otherwise vmax is not touched and the denominator uses v)
 *     den = sqrt(vmax) / bias_correction2_sqrt + eps
 *     p  = p - step_size * (m / den)
 * NaN and Inf propagate as the formulas say; max gives NaN when either side is NaN (torch.maximum).  Subnormals are kept.
 * `aligned` != 0 promises that all five pointers of the chunk (four without amsgrad) are 16-byte aligned: whole groups of four
 * elements then move as 16-byte loads and stores and the last n % 4 elements one by one; `aligned` == 0 (a gradient that is a view
 * into a flat reduction bucket at any element offset) moves every element on its own.  Both paths compute the same roundings.
 * No workgroup waits for another, no atomics, no scratch memory; every access through a table pointer is a global access.
 * partial_sq, NULL or a device float64 [n_chunks] array: chunk i also stores sum(double(g) * double(g)) over its elements (the
 * RAW gradient, before weight decay; squares of floats are exact in float64) at partial_sq[i] -- each lane adds its elements in
 * index order, then a fixed tree over the workgroup: the same bits run after run.
 * The host rounds every float of bmc_adam_hyper_t ONCE from the float64 values torch's _single_tensor_adam computes for step t:
 * step_size = lr / (1 - beta1^t), bias_correction2_sqrt = (1 - beta2^t)^0.5. */
#define BMC_ADAM_CHUNK 4096
typedef struct bmc_adam_chunk {
    float* p;
    const float* g;
    float* m;               /* exp_avg */
    float* v;               /* exp_avg_sq */
    float* vmax;            /* max_exp_avg_sq; NULL without amsgrad */
    int n;                  /* 1 .. BMC_ADAM_CHUNK elements */
    int aligned;
} bmc_adam_chunk_t;
typedef struct bmc_adam_hyper {
    double lr, beta1_f64, beta2_f64;    /* read by the capturable entry point only */
    float beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
    float step_size, bias_correction2_sqrt;     /* ignored by the capturable entry point */
    int amsgrad;
} bmc_adam_hyper_t;
/* Checked: n_chunks >= 0 (0: nothing is launched), a table when n_chunks > 0, every hyper-parameter the entry point reads
 * finite.  Trusted: the table's pointers, counts and flags. */
int bmc_adam_step(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, double* partial_sq, bmc_stream_t s);
/* The same pass for a captured graph, TWO launches.  step_dev is a device int32.  The first launch reads t = *step_dev + 1; one
 * lane per workgroup computes step_size = lr / (1 - beta1_f64^t) and bias_correction2_sqrt = sqrt(1 - beta2_f64^t) in float64 and
 * rounds them to float32; the pass then runs as above.  The second launch (one lane) stores t to *step_dev.  lr, beta1_f64 and
 * beta2_f64 are baked into the graph. */
int bmc_adam_step_capturable(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, int* step_dev, double* partial_sq,
                             bmc_stream_t s);

/* ---- optimizer step: clipping (bmcnet-esr_amd/bmc_hip/optim.py::Adam(max_grad_norm=, nonfinite=); csrc/optim.hip) ---------------
 * Clipping by the GLOBAL L2 norm of all gradients of a step (torch.nn.utils.clip_grad_norm_ followed by Adam.step()) and the skip
 * of a step whose gradients are not finite, with no host round trip.  A clipped step of one optimizer is k NORM launches followed
 * by k STEP launches over the same k chunk tables, k being the launches of an unclipped step (one per group and step-count cohort,
 * normally 1).  The partials of all k norm launches share ONE float64 array of n_partials entries; launch j writes its n_chunks
 * entries at its offset, and every step launch reads the whole array.
 * Norm launch, bmc_adam_grad_sq: grid n_chunks workgroups of 256 lanes; chunk i stores sum(double(g) * double(g)) over its
 * elements at partial_sq[i], with the lane-to-element assignment (aligned and element-wise path alike), the per-lane order and the
 * fixed LDS tree of the step kernel above: for one table the values are BIT-IDENTICAL to what bmc_adam_step(..., partial_sq, ...)
 * stores.  It reads g only and writes nothing but partial_sq[0 .. n_chunks).
 * Step launch: every workgroup first forms the same total -- lane t adds partial_sq[t], partial_sq[t + 256], ... in that order in
 * float64, then the same fixed tree -- so all workgroups hold identical bits.  Then, each line ONE rounding, no fused multiply-add:
 *     norm = sqrt(total)                float64
 *     n32  = (float) norm
 *     s    = n32 + 1e-6f                float32
 *     q    = max_norm / s               float32, IEEE division
 *     c    = (q > 1.0f) ? 1.0f : q      a NaN q stays NaN (torch.clamp(max=1.0))
 *     g_c  = g * c                      float32; g itself is never written
 * and the six lines of "optimizer step" run on g_c (weight decay is added AFTER clipping, as when one clips before torch's step()).
 * Both step kernels run the same walk and element function (csrc/adam_k.h): for c == 1.0f the results are bit-identical to
 * bmc_adam_step's.  max_norm = +INF never clips (c = 1 for every finite total).
 * Non-finite totals.  Squares of float32 values cannot overflow float64: the total is not finite exactly when some gradient
 * element is Inf or NaN.  skip_nonfinite == 0: the formulas decide -- an Inf total gives c = 0 (finite gradients become 0, Inf
 * elements NaN), a NaN total gives c = NaN (everything becomes NaN): clip_grad_norm_(error_if_nonfinite=False).  skip_nonfinite == 1
 * and a non-finite total: no workgroup stores anything to p, m, v or vmax (the branch is uniform over the grid).
 * info, NULL or a device double[2]: workgroup 0 stores info[0] = norm, info[1] = (double) c, also for a skipped step.  skipped,
 * NULL or a device int32: when the step is skipped, workgroup 0 does *skipped += 1.  Both are plain stores by one lane.  The host
 * passes info and skipped to the FIRST step launch of a step only.
 * The clipped entry points have no partial_sq output of their own: the norm launches' array is the gradient norm's partials.
 * Capturable form: the step count comes from *step_dev as in bmc_adam_step_capturable, and the advance launch follows the step
 * launch ALSO for a skipped step: a skipped step counts as a step, on the host and on the device (nothing on the host can know
 * otherwise without a sync), so the bias corrections of later steps see t one higher than the number of updates applied.
 * Checked: n_chunks >= 0, tables and partial_sq non-NULL where n_chunks > 0, n_partials >= n_chunks, max_norm > 0 and not NaN,
 * skip_nonfinite 0 or 1, and the hyper-parameter checks above.  Trusted: the tables.  No flat access, no scratch, no atomics, no
 * workgroup waits for another. */
typedef struct bmc_adam_clip {
    const double* partial_sq;   /* the whole partials array of the step */
    double* info;               /* NULL or double[2]: {norm, c} */
    int* skipped;               /* NULL or int32: += 1 when the step is skipped */
    int n_partials;             /* length of partial_sq */
    float max_norm;             /* > 0; +INF: never clip */
    int skip_nonfinite;         /* 0 or 1 */
} bmc_adam_clip_t;
int bmc_adam_grad_sq(const bmc_adam_chunk_t* table, int n_chunks, double* partial_sq, bmc_stream_t s);
int bmc_adam_step_clipped(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, bmc_adam_clip_t clip, bmc_stream_t s);
int bmc_adam_step_clipped_capturable(const bmc_adam_chunk_t* table, int n_chunks, bmc_adam_hyper_t hyper, int* step_dev,
                                     bmc_adam_clip_t clip, bmc_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* BMC_HIP_H */
