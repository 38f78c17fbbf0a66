// Hot-pixel filter of event-backed multi-stream inference (bmcnet-esr_amd/infer.py::MultiStreamSR(hot_filter=...)); the contract
// is stated once in include/bmc_hip.h ("hot-pixel filter").  Per window and for all slots in ONE launch, bmc_slot_hot_update
// folds every newly observed LR item into the slot's running per-pixel counts and selects the item's mask by the rule of the
// reference's get_hot_event_mask (dataloader/encodings.py:349-364, fed by create_hot_mask, dataloader/h5dataset.py:528-548);
// bmc_hot_pixel_mask is the same selection on a plain float32 rate image (the drop-in bmc_hip.encodings.get_hot_event_mask).
//
// One workgroup of 1 024 lanes owns a slot (a 180 x 240 frame is 43 pixels per lane), so no workgroup ever waits for another and
// the phases of an item are separated by workgroup barriers only:
//   observe  ws[pixel] = the largest event index that maps to the pixel (integer atomicMax: the LAST event in column order wins,
//            the technique of bmc_events_to_mask), then obs = |p| of that event (0 for an out-of-range event, which maps to (0, 0));
//   count    counts += obs (counts = obs for the first item after a reset);
//   select   on unsigned integer keys (the counts; a monotone image of the floats for bmc_hot_pixel_mask): the pixels with
//            key >= kmin are candidates.  At most max_px of them: all are masked (one counting pass -- the common case).  More:
//            an 8-bit radix select over LDS histograms finds the max_px-th largest key T, every key > T is masked and, of the
//            keys == T, the first ones in flat order (an ordered prefix count: a contiguous chunk per lane, then wave_k.h's
//            block_scan_excl over the lanes);
//   write    the item's mask into the slot's ring and, for the window's last item, into the recording's own outputs.
// Integers only in every decision, no atomics whose order matters, grid fixed by S: the same bytes run after run, capturable.
// Pointers read from the tables go through address-space(1) casts (global_* instructions, never flat_*), as in slot_events.hip.
#include "bmc_common.h"
#include "slot_encode_k.h"
#include "wave_k.h"

namespace {

constexpr int HT = 1024;            // threads per workgroup
constexpr int HNW = HT / 64;

struct Lds {
    unsigned hist[256];
    unsigned red[HNW];
    unsigned sel[2];
};

// op(a, b) over the workgroup; every lane gets the result.  red is used again and again: the leading barrier ends its
// previous reading
template <class Op>
__device__ __forceinline__ unsigned block_reduce(unsigned v, Lds& l, Op op) {
    __syncthreads();
    return block_fold_all<HNW>(v, op, l.red);
}
__device__ __forceinline__ unsigned block_sum(unsigned v, Lds& l) { return block_reduce(v, l, Sum()); }
__device__ __forceinline__ unsigned block_min(unsigned v, Lds& l) { return block_reduce(v, l, Min()); }
__device__ __forceinline__ unsigned block_max(unsigned v, Lds& l) { return block_reduce(v, l, Max()); }

// What to mask: every key > T; of the keys == T the first need_eq in flat order; and pixel `extra` (or none: -1).
struct Decision {
    unsigned T, need_eq;
    int extra;
};
__device__ __forceinline__ Decision keep_all() { return Decision{0xffffffffu, 0u, -1}; }

// Rule 3 of the contract on keys[0 .. n) (global memory, written by this workgroup before a barrier).  kmin >= 1.
// neg (max_rate < 0): kmin is the key above zero, and the reference's loop, which re-finds the entries it has zeroed, spends
// what is left of max_px on ONE more pixel: the first in flat order with key >= zero_key, else (every value negative) the
// first maximum if it reaches ext_kmin.
__device__ __forceinline__ Decision select(const unsigned* keys, int n, unsigned kmin, int max_px, int neg, unsigned zero_key, unsigned ext_kmin,
                           Lds& l) {
    const int tid = threadIdx.x;
    Decision d = keep_all();
    if (max_px <= 0) return d;
    unsigned c = 0u;
    for (int p = tid; p < n; p += HT) c += gld<unsigned>(keys + p) >= kmin ? 1u : 0u;
    const unsigned ncand = block_sum(c, l);
    if (ncand <= (unsigned)max_px) {
        d.T = kmin - 1u;
        if (neg && ncand < (unsigned)max_px) {
            unsigned first = (unsigned)n;
            for (int p = tid; p < n; p += HT)
                if (gld<unsigned>(keys + p) >= zero_key) { first = (unsigned)p; break; }
            first = block_min(first, l);
            if (first == (unsigned)n) {
                unsigned mx = 0u;
                for (int p = tid; p < n; p += HT) { const unsigned k = gld<unsigned>(keys + p); mx = k > mx ? k : mx; }
                mx = block_max(mx, l);
                if (mx >= ext_kmin) {
                    for (int p = tid; p < n; p += HT)
                        if (gld<unsigned>(keys + p) == mx) { first = (unsigned)p; break; }
                    first = block_min(first, l);
                }
            }
            if (first < (unsigned)n) d.extra = (int)first;
        }
        return d;
    }
    // more candidates than max_px: the max_px-th largest key, digit by digit from the top.  The largest comes first: digit dg
    // counts into the mirrored bin 255 - dg, and wave 0 picks the bin of the 0-based rank k - 1 from bin 0 (digit_pick)
    unsigned prefix = 0u, pmask = 0u, k = (unsigned)max_px;
    for (int shift = 24; shift >= 0; shift -= 8) {
        __syncthreads();
        if (tid < 256) l.hist[tid] = 0u;
        __syncthreads();
        for (int p = tid; p < n; p += HT) {
            const unsigned key = gld<unsigned>(keys + p);
            if ((key & pmask) == prefix) atomicAdd(&l.hist[(~key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {
            const DigitPick dp = digit_pick(l.hist, k - 1u, tid);
            if (dp.found) { l.sel[0] = 255u - dp.bin; l.sel[1] = dp.rank + 1u; }
        }
        __syncthreads();
        prefix |= l.sel[0] << shift;
        pmask |= 255u << shift;
        k = l.sel[1];
    }
    d.T = prefix;
    d.need_eq = k;
    return d;
}

// out(p, masked) for every pixel; -> the number of masked pixels (on every lane)
template <class F>
__device__ unsigned apply(const unsigned* keys, int n, const Decision& d, Lds& l, F out) {
    const int tid = threadIdx.x;
    unsigned nm = 0u;
    if (d.need_eq == 0u) {
        for (int p = tid; p < n; p += HT) {
            const bool m = gld<unsigned>(keys + p) > d.T || p == d.extra;
            nm += m ? 1u : 0u;
            out(p, m);
        }
        return block_sum(nm, l);
    }
    const int chunk = (n + HT - 1) / HT;
    const long long lo64 = (long long)tid * chunk;
    const int lo = (int)(lo64 < n ? lo64 : n), hi = (int)(lo64 + chunk < n ? lo64 + chunk : n);
    unsigned eq = 0u;
    for (int p = lo; p < hi; ++p) eq += gld<unsigned>(keys + p) == d.T ? 1u : 0u;
    __syncthreads();                                                 // (the previous reader of red is done)
    unsigned all, before = block_scan_excl<HNW>(eq, l.red, &all);    // the keys == T of the lanes below, in flat order
    for (int p = lo; p < hi; ++p) {
        const unsigned key = gld<unsigned>(keys + p);
        bool m = key > d.T || p == d.extra;
        if (key == d.T) m = m || before++ < d.need_eq;
        nm += m ? 1u : 0u;
        out(p, m);
    }
    return block_sum(nm, l);
}

// grid (S): one workgroup per slot
__global__ __launch_bounds__(HT) void slot_hot_update_kernel(const bmc_slot_hot_t* __restrict__ hot,
                                                             const bmc_slot_events_t* __restrict__ events, int seqn, int H, int W,
                                                             int max_px, int neg, int* __restrict__ counts,
                                                             unsigned char* __restrict__ ring, int* __restrict__ ws) {
    __shared__ Lds l;
    const int s = blockIdx.x, tid = threadIdx.x, n = H * W;
    const bmc_slot_hot_t* const ent = hot + s;
    if (!gld<int>(&ent->active)) return;                             // not filtered: nothing of the slot is touched
    const bmc_slot_events_t* const ev = events + s;
    const short* const xs = gld<const short*>(&ev->lr_xs);
    const short* const ys = gld<const short*>(&ev->lr_ys);
    const double* const ps = gld<const double*>(&ev->lr_ps);
    if (xs == nullptr) return;
    const int first_item = gld<int>(&ent->first_item), new_from = gld<int>(&ent->new_from);
    int* const hot_pixels = gld<int*>(&ent->hot_pixels);
    unsigned char* const hot_mask = gld<unsigned char*>(&ent->hot_mask);
    int* const cnt = counts + (long long)s * n;
    int* const own = ws + (long long)s * n;
    for (int t = new_from < 0 ? 0 : new_from; t < seqn; ++t) {
        const long long e0 = gld<long long>(&ev->lr_range[t][0]), e1 = gld<long long>(&ev->lr_range[t][1]);
        for (int p = tid; p < n; p += HT) own[p] = -1;
        __syncthreads();
        for (long long e = e0 + tid; e < e1; e += HT) {
            const int x = (int)gld<short>(xs + e), y = (int)gld<short>(ys + e);
            const bool oob = x < 0 || x >= W || y < 0 || y >= H;
            atomicMax(own + (oob ? 0 : y * W + x), (int)(e - e0));
        }
        __syncthreads();
        const bool fresh = t == 0 && new_from == 0;                  // a reset slot: whatever the counts held is forgotten
        for (int p = tid; p < n; p += HT) {
            // the winners were written by atomics, which execute in L2: read them there, past a line this CU may still hold
            const int w = __hip_atomic_load(own + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int obs = 0;
            if (w >= 0) {
                const long long e = e0 + w;
                const int x = (int)gld<short>(xs + e), y = (int)gld<short>(ys + e);
                const bool oob = x < 0 || x >= W || y < 0 || y >= H;
                obs = !oob && gld<double>(ps + e) != 0.0 ? 1 : 0;
            }
            cnt[p] = (fresh ? 0 : cnt[p]) + obs;
        }
        __syncthreads();
        const int cmin = gld<int>(&ent->cmin[t]);
        const Decision d = cmin < 1 ? keep_all() : select((const unsigned*)cnt, n, (unsigned)cmin, max_px, neg, 0u, 0u, l);
        unsigned char* const m = ring + ((long long)s * seqn + (first_item + t) % seqn) * n;
        const bool last = t == seqn - 1;
        const unsigned nm = apply((const unsigned*)cnt, n, d, l, [&](int p, bool masked) {
            m[p] = masked ? 0 : 1;
            if (last && hot_mask) gst<unsigned char>(hot_mask + p, masked ? 0 : 1);
        });
        if (last && hot_pixels && tid == 0) gst<int>(hot_pixels, (int)nm);
        __syncthreads();
    }
}

__device__ __forceinline__ unsigned float_key(float v) {
    unsigned b = v == 0.f ? 0u : __float_as_uint(v);                 // -0.0 orders as +0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static unsigned float_key_host(float v) {
    unsigned b = 0u;
    if (v != 0.f) __builtin_memcpy(&b, &v, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// one workgroup: the selection on the monotone unsigned image of a float32 rate image
__global__ __launch_bounds__(HT) void hot_pixel_mask_kernel(float* __restrict__ rate, int n, int active, int max_px, unsigned kmin,
                                                            int neg, unsigned ext_kmin, float* __restrict__ mask,
                                                            unsigned* __restrict__ keys) {
    __shared__ Lds l;
    const int tid = threadIdx.x;
    unsigned nan = 0u;
    for (int p = tid; p < n; p += HT) {
        const float v = rate[p];
        nan |= v != v ? 1u : 0u;
        keys[p] = float_key(v);
    }
    nan = block_max(nan, l);                                         // (its barriers also publish the keys)
    // a NaN is the first maximum argmax finds and is not > max_rate: the reference's loop stops before it masks anything
    const Decision d = (!active || nan) ? keep_all() : select(keys, n, kmin, max_px, neg, 0x80000000u, ext_kmin, l);
    apply(keys, n, d, l, [&](int p, bool masked) {
        mask[p] = masked ? 0.f : 1.f;
        if (masked) rate[p] = 0.f;
    });
}

// bmc_slot_encode's grid; the LR bands of filtered slots are stored through their item's mask (slot_encode_k.h)
__global__ __launch_bounds__(ET) void slot_encode_filtered_kernel(const bmc_slot_events_t* __restrict__ table, int seqn, int H,
                                                                  int W, int gh, int gw, int r_lr, int nb_lr, int r_gt,
                                                                  float* __restrict__ lr_scratch, float* __restrict__ gt_scratch,
                                                                  const bmc_slot_hot_t* __restrict__ hot,
                                                                  const unsigned char* __restrict__ ring) {
    __shared__ unsigned cnt[ENC_LDS];
    slot_encode_body<true>(cnt, table, seqn, H, W, gh, gw, r_lr, nb_lr, r_gt, lr_scratch, gt_scratch, hot, ring);
}

}  // namespace

extern "C" int bmc_slot_encode_filtered(const bmc_slot_events_t* table, const bmc_slot_hot_t* hot, const unsigned char* ring, int S,
                                        int seqn, int H, int W, int gh, int gw, float* lr_scratch, float* gt_scratch, bmc_stream_t s) {
    BMC_CHECK_ARG(table && hot && ring && lr_scratch && gt_scratch && S >= 1 && S <= BMC_MAX_SLOTS && seqn >= 2 &&
                      seqn <= BMC_SLOT_MAX_SEQN && H > 0 && W > 0 && gh > 0 && gw > 0,
                  "bmc_slot_encode_filtered: bad arguments");
    BMC_CHECK_ARG(2 * W <= ENC_LDS && 2 * gw <= ENC_LDS, "bmc_slot_encode_filtered: frames wider than %d pixels are not supported",
                  ENC_LDS / 2);
    const SlotEncodeGrid g = slot_encode_grid(H, W, gh, gw);
    hipLaunchKernelGGL(slot_encode_filtered_kernel, dim3(seqn * g.nb_lr + g.nb_gt, S), dim3(ET), 0, (hipStream_t)s, table, seqn, H, W,
                       gh, gw, g.r_lr, g.nb_lr, g.r_gt, lr_scratch, gt_scratch, hot, ring);
    BMC_CHECK_LAUNCH("bmc_slot_encode_filtered");
    return 0;
}

extern "C" int bmc_slot_hot_update(const bmc_slot_hot_t* hot, const bmc_slot_events_t* events, int S, int seqn, int H, int W,
                                   int max_px, int negative_rate, int* counts, unsigned char* ring, int* ws, bmc_stream_t s) {
    BMC_CHECK_ARG(hot && events && counts && ring && ws && S >= 1 && S <= BMC_MAX_SLOTS && seqn >= 2 && seqn <= BMC_SLOT_MAX_SEQN &&
                      H > 0 && W > 0 && max_px >= 0,
                  "bmc_slot_hot_update: bad arguments");
    BMC_CHECK_ARG((long long)H * W < (1ll << 30), "bmc_slot_hot_update: frames of %d x %d pixels are not supported", H, W);
    hipLaunchKernelGGL(slot_hot_update_kernel, dim3(S), dim3(HT), 0, (hipStream_t)s, hot, events, seqn, H, W, max_px,
                       negative_rate ? 1 : 0, counts, ring, ws);
    BMC_CHECK_LAUNCH("bmc_slot_hot_update");
    return 0;
}

extern "C" int bmc_hot_pixel_mask(float* event_rate, int H, int W, int active, int max_px, float max_rate, float* mask,
                                  unsigned* ws, bmc_stream_t s) {
    BMC_CHECK_ARG(event_rate && mask && ws && H > 0 && W > 0 && max_px >= 0, "bmc_hot_pixel_mask: bad arguments");
    BMC_CHECK_ARG((long long)H * W < (1ll << 30), "bmc_hot_pixel_mask: images of %d x %d pixels are not supported", H, W);
    if (max_rate != max_rate) active = 0;                            // nothing is > NaN
    const int neg = max_rate < 0.f;
    const unsigned above = float_key_host(active ? max_rate : 0.f) + 1u;     // the smallest key of a value > max_rate
    hipLaunchKernelGGL(hot_pixel_mask_kernel, dim3(1), dim3(HT), 0, (hipStream_t)s, event_rate, H * W, active ? 1 : 0, max_px,
                       neg ? 0x80000001u : above, neg, above, mask, ws);
    BMC_CHECK_LAUNCH("bmc_hot_pixel_mask");
    return 0;
}
