// The body of the slot encode kernels (internal): slot_encode_kernel (slot_events.hip, bmc_slot_encode) and
// slot_encode_filtered_kernel (slot_hot.hip, bmc_slot_encode_filtered) are its two instantiations.  slot_events.hip describes
// the algorithm.
#pragma once
#include "slot_k.h"

namespace {

constexpr int ET = 1024;            // threads per workgroup
constexpr int ENC_LDS = 15360;      // counters per workgroup: 2 channels x R rows x W (60 KB: two workgroups per CU)

// rows per band and bands per frame of the launch: grid (seqn * nb_lr + nb_gt, S)
struct SlotEncodeGrid {
    int r_lr, nb_lr, r_gt, nb_gt;
};
static inline SlotEncodeGrid slot_encode_grid(int H, int W, int gh, int gw) {
    SlotEncodeGrid g;
    g.r_lr = ENC_LDS / (2 * W) < H ? ENC_LDS / (2 * W) : H;
    g.r_gt = ENC_LDS / (2 * gw) < gh ? ENC_LDS / (2 * gw) : gh;
    g.nb_lr = (H + g.r_lr - 1) / g.r_lr;
    g.nb_gt = (gh + g.r_gt - 1) / g.r_gt;
    return g;
}

// The body of both encode kernels.  HOT (bmc_slot_encode_filtered; the contract: include/bmc_hip.h "hot-pixel filter", rule 4): an
// LR band of a slot with an active hot entry is multiplied by its item's mask as it is stored -- mask row H-1-row for output row
// `row`, both channels; ground-truth bands and slots without an active entry are stored as without HOT.
template <bool HOT>
__device__ __forceinline__ void slot_encode_body(unsigned* cnt, const bmc_slot_events_t* __restrict__ table, int seqn, int H, int W,
                                                 int gh, int gw, int r_lr, int nb_lr, int r_gt, float* __restrict__ lr_scratch,
                                                 float* __restrict__ gt_scratch, const bmc_slot_hot_t* __restrict__ hot,
                                                 const unsigned char* __restrict__ ring) {
    const int s = blockIdx.y, tid = threadIdx.x;
    const bmc_slot_events_t* const ent = table + s;
    if (gld<const short*>(&ent->lr_xs) == nullptr) return;           // no event entry: the slot's scratch is not touched
    const short *xs, *ys;
    const double* ps;
    long long e0, e1;
    int fh, fw, r0, rows;
    float* out;
    const unsigned char* mask = nullptr;
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
        if constexpr (HOT) {
            if (gld<int>(&hot[s].active))
                mask = ring + ((long long)s * seqn + (gld<int>(&hot[s].first_item) + t) % seqn) * H * W;
        }
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
    if constexpr (HOT) {
        if (mask != nullptr) {
            for (int i = tid; i < n; i += ET) {
                const int rr = i / fw;
                const unsigned keep = mask[(long long)(fh - 1 - (r0 + rr)) * fw + (i - rr * fw)] ? 1u : 0u;
                gst<float>(o0 + i, (float)(cnt[i] * keep));
                gst<float>(o1 + i, (float)(cnt[n + i] * keep));
            }
            return;
        }
    }
    for (int i = tid; i < n; i += ET) {
        gst<float>(o0 + i, (float)cnt[i]);
        gst<float>(o1 + i, (float)cnt[n + i]);
    }
}

}  // namespace
