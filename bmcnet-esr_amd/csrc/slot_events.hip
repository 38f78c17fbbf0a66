// Event-backed recording slots of multi-stream inference (bmcnet-esr_amd/infer.py::MultiStreamSR.open_events): the recording
// stays on the GPU as raw dataset columns (xs / ys int16, ps float64) and bmc_slot_encode builds, per window and for all slots
// in ONE launch, the count images that bmc_slot_stage / bmc_slot_metrics then read from per-slot scratch: the window's seqn LR
// frames and its one ground-truth frame (what H5Dataset.__getitem__ does per item on the CPU, dataloader/h5dataset.py:261-316,
// without augmentation -- the arithmetic of scatter.hip's encode_raw_kernel with flips = 0, out-of-range quirk included).
//
// A workgroup owns a band of R rows (both channels) of one output frame: it zeroes the band in LDS, scans ALL events of that
// frame (2 048 for an LR frame, 32 768 for a x4 ground truth: a few hundred KB that stay in L2 while the frame's bands run),
// counts the ones that land in its band with integer LDS atomics and stores the band once -- the store is the zero fill, so
// there is no memset launch and no float atomic on global memory.  Only the row decides the band, so a lane reads ys first
// (2 bytes per event) and xs / ps only for events that can land in the band.  Counts are integers: the result does not
// depend on the order of the atomics and is the same bits run after run.
// Pointers read from the table go through address-space(1) casts (global_* instructions, never flat_*), as in slots.hip.
#include "bmc_common.h"

namespace {

template <class T>
__device__ __forceinline__ T gld(const void* p) {
    return *(const __attribute__((address_space(1))) T*)(unsigned long long)p;
}
template <class T>
__device__ __forceinline__ void gst(void* p, T v) {
    *(__attribute__((address_space(1))) T*)(unsigned long long)p = v;
}

constexpr int ET = 1024;            // threads per workgroup
constexpr int ENC_LDS = 15360;      // counters per workgroup: 2 channels x R rows x W (60 KB: two workgroups per CU)

// grid (seqn * nb_lr + nb_gt, S): blockIdx.y is the slot, blockIdx.x a (frame, band) of that slot's window
__global__ __launch_bounds__(ET) void slot_encode_kernel(const bmc_slot_events_t* __restrict__ table, int seqn, int H, int W,
                                                         int gh, int gw, int r_lr, int nb_lr, int r_gt,
                                                         float* __restrict__ lr_scratch, float* __restrict__ gt_scratch) {
    __shared__ unsigned cnt[ENC_LDS];
    const int s = blockIdx.y, tid = threadIdx.x;
    const bmc_slot_events_t* const ent = table + s;
    if (gld<const short*>(&ent->lr_xs) == nullptr) return;           // no event entry: the slot's scratch is not touched
    const short *xs, *ys;
    const double* ps;
    long long e0, e1;
    int fh, fw, r0, rows;
    float* out;
    const int b = blockIdx.x;
    if (b < seqn * nb_lr) {
        const int t = b / nb_lr;
        xs = gld<const short*>(&ent->lr_xs);
        ys = gld<const short*>(&ent->lr_ys);
        ps = gld<const double*>(&ent->lr_ps);
        e0 = gld<long long>(&ent->lr_range[t][0]);
        e1 = gld<long long>(&ent->lr_range[t][1]);
        fh = H; fw = W; r0 = (b - t * nb_lr) * r_lr; rows = r_lr;
        out = lr_scratch + ((long long)s * seqn + t) * 2 * H * W;
    } else {
        xs = gld<const short*>(&ent->gt_xs);
        ys = gld<const short*>(&ent->gt_ys);
        ps = gld<const double*>(&ent->gt_ps);
        e0 = gld<long long>(&ent->gt_range[0]);
        e1 = gld<long long>(&ent->gt_range[1]);
        fh = gh; fw = gw; r0 = (b - seqn * nb_lr) * r_gt; rows = r_gt;
        out = gt_scratch + (long long)s * 2 * gh * gw;
    }
    if (r0 + rows > fh) rows = fh - r0;
    const int n = rows * fw;                                         // counters per channel: 2 * n <= ENC_LDS
    for (int i = tid; i < 2 * n; i += ET) cnt[i] = 0u;
    __syncthreads();
    const bool last = r0 + rows == fh;                               // row fh-1 is where out-of-range negatives land
    for (long long e = e0 + tid; e < e1; e += ET) {
        // event_formatting's float32 cast of the int16 column is exact, so the range tests run on the integers
        const int y = (int)gld<short>(ys + e);
        const bool yin = y >= 0 && y < fh;
        const int row = fh - 1 - (yin ? y : 0);
        if (!(last || (yin && row >= r0 && row < r0 + rows))) continue;
        const int x = (int)gld<short>(xs + e);
        const float p = (float)gld<double>(ps + e);
        const bool oob = !yin || x < 0 || x >= fw;
        const bool neg = p < 0.f;
        if (!(neg || (!oob && p > 0.f))) continue;                   // an out-of-range positive (or p = 0) counts nowhere
        const int rr = (oob ? fh - 1 : row) - r0;                    // reset coordinates (0, 0) -> [fh-1][0] of channel 1
        if (rr < 0 || rr >= rows) continue;
        atomicAdd(&cnt[(neg ? n : 0) + rr * fw + (oob ? 0 : x)], (unsigned)(p * p));
    }
    __syncthreads();
    float* const o0 = out + (long long)r0 * fw;
    float* const o1 = o0 + (long long)fh * fw;
    for (int i = tid; i < n; i += ET) {
        gst<float>(o0 + i, (float)cnt[i]);
        gst<float>(o1 + i, (float)cnt[n + i]);
    }
}

}  // namespace

extern "C" int bmc_slot_encode(const bmc_slot_events_t* table, int S, int seqn, int H, int W, int gh, int gw, float* lr_scratch,
                               float* gt_scratch, bmc_stream_t s) {
    BMC_CHECK_ARG(table && lr_scratch && gt_scratch && S >= 1 && S <= BMC_MAX_SLOTS && seqn >= 2 && seqn <= BMC_SLOT_MAX_SEQN &&
                      H > 0 && W > 0 && gh > 0 && gw > 0,
                  "bmc_slot_encode: bad arguments");
    BMC_CHECK_ARG(2 * W <= ENC_LDS && 2 * gw <= ENC_LDS, "bmc_slot_encode: frames wider than %d pixels are not supported",
                  ENC_LDS / 2);
    const int r_lr = ENC_LDS / (2 * W) < H ? ENC_LDS / (2 * W) : H, r_gt = ENC_LDS / (2 * gw) < gh ? ENC_LDS / (2 * gw) : gh;
    const int nb_lr = (H + r_lr - 1) / r_lr, nb_gt = (gh + r_gt - 1) / r_gt;
    hipLaunchKernelGGL(slot_encode_kernel, dim3(seqn * nb_lr + nb_gt, S), dim3(ET), 0, (hipStream_t)s, table, seqn, H, W, gh, gw,
                       r_lr, nb_lr, r_gt, lr_scratch, gt_scratch);
    BMC_CHECK_LAUNCH("bmc_slot_encode");
    return 0;
}
