// Sequence encoder for training (bmcnet-esr_amd/event_dataset.py::EventTrainSet.batch): recordings stay on the GPU as raw
// dataset columns and bmc_seq_encode builds, in ONE launch per batch, every LR and HR count image of B sequences of L items in
// the collate layout -- what SequenceDataset.__getitem__ (dataloader/h5dataset.py:666-700) has H5Dataset.__getitem__ (:261-316)
// do per item in the loader's worker processes: flips shared by the sequence, paused items, noise events.  The contract:
// include/bmc_hip.h "sequence encoder for training".
//
// The scheme is slot_events.hip's (slot_encode_k.h): a workgroup owns a band of R rows (both channels) of one output frame,
// zeroes it in LDS, scans the frame's events -- ys first, xs / ps only for events that can land in the band -- counts with
// integer LDS atomics and stores the band once; the store is the zero fill.  No global atomics, no memset, no workgroup waits
// for another; counts are integers, so the result does not depend on the order of the atomics.  The differences: a frame per
// item for the ground truth too, the flips applied to the int16 coordinates and the polarity before the range test, a
// paused LR item that scans nothing, and the sample's noise events counted (unflipped) on top of every LR item that runs.
//
// bmc_seq_encode_crop (EventTrainSet(crop=...)) is the same body writing one patch per sample: the output frame is the patch,
// the flips and the range test keep the sample's own full frame, and an event counts when its full-frame pixel lies in the band.
// Bit 3 of a sample's flips transposes its frames (with the two flips: all 8 orientations of a patch): the patch is cut out
// of the TRANSPOSED full frame, so x is the coordinate that picks the row -- tested first -- and fh-1-y the column; the
// out-of-range negatives land at [0][fh-1].  The choice is the sample's, uniform per workgroup; bmc_seq_encode ignores the bit.
#include "bmc_common.h"
#include "slot_encode_k.h"

namespace {

// One event whose row test has passed (or whose band holds the landing pixel of the out-of-range negatives): the arithmetic of
// slot_encode_body, on the flipped values.  (row, col): the event's pixel in the output orientation of the full frame, (qr, qc)
// the landing pixel there -- [fh-1][0], transposed [0][fh-1].  The band starts at row f0 and, with CROP, at column `left`; it has
// `rows` rows of pw pixels.
template <bool CROP>
__device__ __forceinline__ void seq_count(unsigned* cnt, bool oob, int row, int col, float p, int qr, int qc, int f0, int rows, int n,
                                          int left, int pw) {
    const bool neg = p < 0.f;
    if (!(neg || (!oob && p > 0.f))) return;                         // an out-of-range positive (or p = 0) counts nowhere
    const int rr = (oob ? qr : row) - f0;                            // reset coordinates (0, 0) -> [fh-1][0] of channel 1
    if (rr < 0 || rr >= rows) return;
    int c = oob ? qc : col;
    if constexpr (CROP) {
        c -= left;
        if (c < 0 || c >= pw) return;
    }
    atomicAdd(&cnt[(neg ? n : 0) + rr * pw + c], (unsigned)(p * p));
}

// A band's scan of its item's events and of the sample's noise.  TR (CROP only): the sample is transposed, so the coordinate that
// picks the row -- the one read first, of every event -- is x against fw, and y picks the column; else y against fh picks the row.
// One instantiation each, so that an untransposed sample runs the code it always ran.
template <bool CROP, bool TR>
__device__ __forceinline__ void seq_scan(unsigned* cnt, const bmc_seq_sample_t* ent, const short* xs, const short* ys, const double* ps,
                                         long long e0, long long e1, int n_noise, unsigned fl, int fh, int fw, int f0, int rows, int n,
                                         int left, int pw) {
    static_assert(CROP || !TR, "full frames have one size per launch: bmc_seq_encode ignores bit 3");
    const int tid = threadIdx.x;
    const int na = TR ? fw : fh, nb = TR ? fh : fw;
    const int qr = TR ? 0 : fh - 1, qc = TR ? fh - 1 : 0;            // where out-of-range negatives land: [fh-1][0], transposed
    // only a band that holds that pixel reads the second coordinate and ps of every event
    const bool last = qr >= f0 && qr < f0 + rows && qc >= left && qc < left + pw;
    const bool fx = fl & 1u, fy = fl & 2u, fp = fl & 4u;
    const bool fa = TR ? fx : fy, fb = TR ? fy : fx;
    const short* const as = TR ? xs : ys;
    const short* const bs = TR ? ys : xs;
    for (long long e = e0 + tid; e < e1; e += ET) {
        // augment_event's float64 flip and event_formatting's float32 cast are exact on int16 values: integers throughout
        int a = (int)gld<short>(as + e);
        if (fa) a = na - 1 - a;
        const bool ain = a >= 0 && a < na;
        const int row = TR ? a : fh - 1 - (ain ? a : 0);
        if (!(last || (ain && row >= f0 && row < f0 + rows))) continue;
        int c = (int)gld<short>(bs + e);
        if (fb) c = nb - 1 - c;
        float p = (float)gld<double>(ps + e);
        if (fp) p = -p;
        seq_count<CROP>(cnt, !ain || c < 0 || c >= nb, row, TR ? fh - 1 - c : c, p, qr, qc, f0, rows, n, left, pw);
    }
    if (n_noise > 0) {                                               // concatenated AFTER augment_event: never flipped
        const short* const nx = gld<const short*>(&ent->noise_xs);
        const short* const ny = gld<const short*>(&ent->noise_ys);
        const signed char* const np = gld<const signed char*>(&ent->noise_ps);
        const short* const nas = TR ? nx : ny;
        const short* const nbs = TR ? ny : nx;
        for (int e = tid; e < n_noise; e += ET) {
            const int a = (int)gld<short>(nas + e);
            const bool ain = a >= 0 && a < na;
            const int row = TR ? a : fh - 1 - (ain ? a : 0);
            if (!(last || (ain && row >= f0 && row < f0 + rows))) continue;
            const int c = (int)gld<short>(nbs + e);
            seq_count<CROP>(cnt, !ain || c < 0 || c >= nb, row, TR ? fh - 1 - c : c, (float)gld<signed char>(np + e), qr, qc, f0, rows, n,
                            left, pw);
        }
    }
}

// The body of both kernels.  (H, W), (gh, gw): the OUTPUT frames -- the recording's with CROP false, the LR and HR patch with
// CROP, where the sample's own frame sizes and the patch origin come from crops[s].
// grid (L * (nb_lr + nb_gt), B): blockIdx.y is the sample, blockIdx.x a (frame, band): first the L * nb_lr LR bands, then the
// L * nb_gt HR bands
template <bool CROP>
__device__ __forceinline__ void seq_encode_body(unsigned* cnt, const bmc_seq_sample_t* __restrict__ table,
                                                const bmc_seq_crop_t* __restrict__ crops, int L, int H, int W, int gh, int gw, int scale,
                                                int r_lr, int nb_lr, int r_gt, int nb_gt, float* __restrict__ inp_cnt,
                                                float* __restrict__ gt_cnt) {
    const int s = blockIdx.y, tid = threadIdx.x;
    const bmc_seq_sample_t* const ent = table + s;
    const unsigned fl = gld<unsigned>(&ent->flips);
    const short *xs, *ys;
    const double* ps;
    long long e0, e1;
    int ph, pw, r0, rows, n_noise = 0;                               // the output frame and the band inside it
    int fh, fw, top = 0, left = 0;                                   // the full frame and where the output frame lies in it
    float* out;
    const int b = blockIdx.x;
    if (b < L * nb_lr) {
        const int t = b / nb_lr;
        xs = gld<const short*>(&ent->lr_xs);
        ys = gld<const short*>(&ent->lr_ys);
        ps = gld<const double*>(&ent->lr_ps);
        e0 = gld<long long>(&ent->lr_range[t][0]);
        e1 = gld<long long>(&ent->lr_range[t][1]);
        ph = H; pw = W; r0 = (b - t * nb_lr) * r_lr; rows = r_lr;
        out = inp_cnt + ((long long)s * L + t) * 2 * H * W;
        if constexpr (CROP) {
            fh = gld<int>(&crops[s].H); fw = gld<int>(&crops[s].W);
            top = gld<int>(&crops[s].top); left = gld<int>(&crops[s].left);
        }
        if ((gld<unsigned>(&ent->paused) >> t) & 1u) e1 = e0;        // a paused item: no events, no noise -> all +0.0
        else n_noise = gld<int>(&ent->n_noise);
    } else {
        const int t = (b - L * nb_lr) / nb_gt;
        xs = gld<const short*>(&ent->gt_xs);
        ys = gld<const short*>(&ent->gt_ys);
        ps = gld<const double*>(&ent->gt_ps);
        e0 = gld<long long>(&ent->gt_range[t][0]);
        e1 = gld<long long>(&ent->gt_range[t][1]);
        ph = gh; pw = gw; r0 = (b - L * nb_lr - t * nb_gt) * r_gt; rows = r_gt;
        out = gt_cnt + ((long long)s * L + t) * 2 * gh * gw;
        if constexpr (CROP) {
            fh = gld<int>(&crops[s].gh); fw = gld<int>(&crops[s].gw);
            top = scale * gld<int>(&crops[s].top); left = scale * gld<int>(&crops[s].left);
        }
    }
    if constexpr (!CROP) { fh = ph; fw = pw; }
    if (r0 + rows > ph) rows = ph - r0;
    const int n = rows * pw;                                         // counters per channel: 2 * n <= ENC_LDS
    for (int i = tid; i < 2 * n; i += ET) cnt[i] = 0u;
    __syncthreads();
    const int f0 = top + r0;                                         // the band's first row in the (transposed) full frame
    bool tr = false;                                                 // the sample's choice: uniform in the workgroup
    if constexpr (CROP) tr = fl & 8u;
    if (tr) {
        if constexpr (CROP) seq_scan<true, true>(cnt, ent, xs, ys, ps, e0, e1, n_noise, fl, fh, fw, f0, rows, n, left, pw);
    } else {
        seq_scan<CROP, false>(cnt, ent, xs, ys, ps, e0, e1, n_noise, fl, fh, fw, f0, rows, n, left, pw);
    }
    __syncthreads();
    float* const o0 = out + (long long)r0 * pw;
    float* const o1 = o0 + (long long)ph * pw;
    for (int i = tid; i < n; i += ET) {
        gst<float>(o0 + i, (float)cnt[i]);
        gst<float>(o1 + i, (float)cnt[n + i]);
    }
}

__global__ __launch_bounds__(ET) void seq_encode_kernel(const bmc_seq_sample_t* __restrict__ table, int L, int H, int W, int gh, int gw,
                                                        int r_lr, int nb_lr, int r_gt, int nb_gt, float* __restrict__ inp_cnt,
                                                        float* __restrict__ gt_cnt) {
    __shared__ unsigned cnt[ENC_LDS];
    seq_encode_body<false>(cnt, table, nullptr, L, H, W, gh, gw, 1, r_lr, nb_lr, r_gt, nb_gt, inp_cnt, gt_cnt);
}

// h x w: the LR patch; the HR patch is scale times it
__global__ __launch_bounds__(ET) void seq_encode_crop_kernel(const bmc_seq_sample_t* __restrict__ table,
                                                             const bmc_seq_crop_t* __restrict__ crops, int L, int h, int w, int scale,
                                                             int r_lr, int nb_lr, int r_gt, int nb_gt, float* __restrict__ inp_cnt,
                                                             float* __restrict__ gt_cnt) {
    __shared__ unsigned cnt[ENC_LDS];
    seq_encode_body<true>(cnt, table, crops, L, h, w, scale * h, scale * w, scale, r_lr, nb_lr, r_gt, nb_gt, inp_cnt, gt_cnt);
}

}  // namespace

extern "C" int bmc_seq_encode(const bmc_seq_sample_t* table, int B, int L, int H, int W, int gh, int gw, float* inp_cnt, float* gt_cnt,
                              bmc_stream_t s) {
    BMC_CHECK_ARG(table && inp_cnt && gt_cnt && B >= 1 && B <= 65535 && L >= 2 && L <= BMC_SEQ_MAX_ITEMS && H > 0 && W > 0 &&
                      gh > 0 && gw > 0,
                  "bmc_seq_encode: bad arguments");
    BMC_CHECK_ARG(2 * W <= ENC_LDS && 2 * gw <= ENC_LDS, "bmc_seq_encode: frames wider than %d pixels are not supported", ENC_LDS / 2);
    const SlotEncodeGrid g = slot_encode_grid(H, W, gh, gw);
    const long long gx = (long long)L * (g.nb_lr + g.nb_gt);
    BMC_CHECK_ARG(gx < (1ll << 31), "bmc_seq_encode: too many bands");
    hipLaunchKernelGGL(seq_encode_kernel, dim3((unsigned)gx, B), dim3(ET), 0, (hipStream_t)s, table, L, H, W, gh, gw, g.r_lr, g.nb_lr,
                       g.r_gt, g.nb_gt, inp_cnt, gt_cnt);
    BMC_CHECK_LAUNCH("bmc_seq_encode");
    return 0;
}

extern "C" int bmc_seq_encode_crop(const bmc_seq_sample_t* table, const bmc_seq_crop_t* crops, int B, int L, int h, int w, int scale,
                                   float* inp_cnt, float* gt_cnt, bmc_stream_t s) {
    BMC_CHECK_ARG(table && crops && inp_cnt && gt_cnt && B >= 1 && B <= 65535 && L >= 2 && L <= BMC_SEQ_MAX_ITEMS && h > 0 && w > 0 &&
                      scale >= 1,
                  "bmc_seq_encode_crop: bad arguments");
    BMC_CHECK_ARG(2ll * scale * w <= ENC_LDS, "bmc_seq_encode_crop: HR patches wider than %d pixels are not supported", ENC_LDS / 2);
    BMC_CHECK_ARG((long long)scale * h < (1ll << 31), "bmc_seq_encode_crop: the HR patch is too tall");
    const SlotEncodeGrid g = slot_encode_grid(h, w, scale * h, scale * w);
    const long long gx = (long long)L * (g.nb_lr + g.nb_gt);
    BMC_CHECK_ARG(gx < (1ll << 31), "bmc_seq_encode_crop: too many bands");
    hipLaunchKernelGGL(seq_encode_crop_kernel, dim3((unsigned)gx, B), dim3(ET), 0, (hipStream_t)s, table, crops, L, h, w, scale, g.r_lr,
                       g.nb_lr, g.r_gt, g.nb_gt, inp_cnt, gt_cnt);
    BMC_CHECK_LAUNCH("bmc_seq_encode_crop");
    return 0;
}
