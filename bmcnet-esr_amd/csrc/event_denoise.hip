// Background-activity noise filter of a raw event stream (bmc_hip.encodings.event_noise_mask, MultiStreamSR.open_events(
// noise_filter=...), EventTrainSet.add_recording(noise_filter=...)); the contract is stated once in include/bmc_hip_denoise.h.
//
// The scheme is slot_encode_kernel's with ordering added.  A workgroup of STEP = 256 lanes owns a band of rows and keeps the
// surface of its band plus one halo row above and below (and one halo column left and right, never written: a pixel outside the
// sensor supports nobody) in LDS as int32 event indices, -1 = none.  Every band walks the whole stream, STEP consecutive events at
// a time, lane l taking event base + l; ys is read first (two steps ahead of the walk), xs and ts one step ahead and only for events
// in band or halo.  Order inside a step, exactly:
//   1  an owning lane reads its eight neighbours from the surface as it stood before the step;
//   2  barrier; every band / halo lane enters its event: atomicMax(last[p], i), and its pixel goes into the step's list pix[lane];
//   3  barrier; the neighbours are read again.  m < base: nobody of this step touched q, the first read stands.  base <= m < i: m
//      is the latest earlier event at q.  m > i: a later lane hid what came before; only then the lane reads pix[] below its own
//      lane (one pass per hidden neighbour, 16 bytes a read) for the latest earlier event of the step at q, and the first
//      read stands if there is none.
// The reads of step 3 and the atomics of the next step's 2 are separated by that step's first barrier: two barriers a step.
// A band writes keep / ps_out for the events whose row it owns (band 0: also for those whose y is out of range), so every element
// is written once and nothing needs a memset.  Integers decide everything but the one float64 subtraction of the contract; no
// global atomic, no workgroup waits for another, grid fixed by (H, W): the same bytes run after run.
#include <math.h>
#include "bmc_common.h"
#include "bmc_hip_denoise.h"
#include "wave_k.h"

namespace {

constexpr int STEP = BMC_DENOISE_STEP;
constexpr int WORDS = BMC_DENOISE_LDS_WORDS;
static_assert(STEP % 64 == 0, "whole waves");

static inline int band_rows(int H, int W) {
    const int r = WORDS / (W + 2) - 2;
    return r < H ? r : H;
}

// grid (ceil(H / R)): one workgroup per band of R rows
__global__ __launch_bounds__(STEP) void event_denoise_kernel(const short* __restrict__ xs, const short* __restrict__ ys,
                                                             const double* __restrict__ ts, const double* __restrict__ ps,
                                                             int n, int H, int W, int R, double dt, int support,
                                                             unsigned char* __restrict__ keep, double* __restrict__ ps_out,
                                                             long long* __restrict__ partial) {
    __shared__ int last[WORDS];
    __shared__ __attribute__((aligned(16))) int pix[STEP];
    __shared__ int wsum[STEP / 64];
    const int tid = threadIdx.x, band = blockIdx.x;
    const int r0 = band * R;
    const int rows = r0 + R > H ? H - r0 : R;
    const int pitch = W + 2;
    for (int p = tid; p < (rows + 2) * pitch; p += STEP) last[p] = -1;
    __syncthreads();
    const int off[8] = {-pitch - 1, -pitch, -pitch + 1, -1, 1, pitch - 1, pitch, pitch + 1};
    int mine = 0;
    // the columns run ahead of the walk: ys two steps, xs and ts (band / halo lanes only) one step
    const auto in_reach = [&](long long e, int y) { return e < n && y >= 0 && y < H && y >= r0 - 1 && y <= r0 + rows; };
    int y_now = tid < n ? (int)gld<short>(ys + tid) : -1;
    int y_next = STEP + tid < n ? (int)gld<short>(ys + STEP + tid) : -1;
    int x_now = -1;
    double t_now = 0.0;
    if (in_reach(tid, y_now)) { x_now = (int)gld<short>(xs + tid); t_now = gld<double>(ts + tid); }
    for (long long base64 = 0; base64 < n; base64 += STEP) {
        const int base = (int)base64;
        const bool valid = base64 + tid < n;
        const int i = valid ? base + tid : 0;
        const int y = y_now, x = x_now;
        const double ti = t_now;
        const long long e1 = base64 + STEP + tid, e2 = e1 + STEP;
        y_now = y_next;
        x_now = -1;
        if (in_reach(e1, y_now)) { x_now = (int)gld<short>(xs + e1); t_now = gld<double>(ts + e1); }
        if (e2 < n) y_next = (int)gld<short>(ys + e2);
        const bool yin = valid && y >= 0 && y < H;
        const bool near = in_reach(base64 + tid, y);
        const bool act = near && x >= 0 && x < W;                    // in range, in band or halo: enters this band's surface
        const bool own = act && y >= r0 && y < r0 + rows;            // ... and is judged here
        const bool writes = valid && (yin ? y >= r0 && y < r0 + rows : band == 0);
        const int p = act ? (y - r0 + 1) * pitch + x + 1 : -1;
        int first[8];
        if (own) {
#pragma unroll
            for (int k = 0; k < 8; ++k) first[k] = last[p + off[k]];
        }
        __syncthreads();
        pix[tid] = p;
        if (act) atomicMax(&last[p], i);
        __syncthreads();
        bool kept = false;
        if (own) {
            int j[8];
            unsigned hidden = 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int m = last[p + off[k]];
                j[k] = first[k];
                if (m >= base) {
                    if (m < i) j[k] = m;
                    else hidden |= 1u << k;
                }
            }
            // one pass over the step's pixel list below this lane per hidden neighbour (most lanes have none, few more than two),
            // four entries a read, in rising order: the last match is the latest
            for (unsigned h = hidden; h; h &= h - 1u) {
                const int k = __ffs((int)h) - 1;
                const int cell = k < 4 ? k : k + 1;                  // of the 3 x 3 block around p, the centre left out: off[k]
                const int q = p + (cell / 3 - 1) * pitch + (cell % 3 - 1);
                int found = -1;
                for (int l0 = 0; l0 < tid; l0 += 4) {
                    const int4 v = *reinterpret_cast<const int4*>(&pix[l0]);
                    if (v.x == q) found = l0;
                    if (v.y == q && l0 + 1 < tid) found = l0 + 1;
                    if (v.z == q && l0 + 2 < tid) found = l0 + 2;
                    if (v.w == q && l0 + 3 < tid) found = l0 + 3;
                }
#pragma unroll
                for (int kk = 0; kk < 8; ++kk)
                    if (kk == k && found >= 0) j[kk] = base + found;
            }
            int c = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (j[k] >= 0) c += ti - gld<double>(ts + j[k]) <= dt ? 1 : 0;
            kept = c >= support;
        }
        if (writes) {
            if (keep) gst<unsigned char>(keep + i, kept ? 1 : 0);
            if (ps_out) gst<double>(ps_out + i, kept ? gld<double>(ps + i) : 0.0);
        }
        mine += kept ? 1 : 0;
    }
    if (partial == nullptr) return;
    mine = block_fold<STEP / 64>(mine, Sum(), wsum);                 // (a band keeps at most n < 2^31 events: no overflow)
    if (tid == 0) gst<long long>(partial + band, (long long)mine);
}

// one workgroup: kept[0] = the sum of the band counts
__global__ __launch_bounds__(STEP) void event_denoise_finish_kernel(const long long* __restrict__ partial, int nb,
                                                                    long long* __restrict__ kept) {
    __shared__ long long wsum[STEP / 64];
    const int tid = threadIdx.x;
    long long v = 0;
    for (int b = tid; b < nb; b += STEP) v += gld<long long>(partial + b);
    v = block_fold<STEP / 64>(v, Sum(), wsum);
    if (tid == 0) gst<long long>(kept, v);
}

}  // namespace

extern "C" int bmc_event_denoise_band_rows(int H, int W) {
    if (H < 1 || W < 1 || W > BMC_DENOISE_MAX_W) return -1;
    return band_rows(H, W);
}

extern "C" long long bmc_event_denoise_scratch_bytes(int H, int W) {
    const int r = bmc_event_denoise_band_rows(H, W);
    return r < 1 ? -1 : 8ll * ((H + r - 1) / r);
}

extern "C" int bmc_event_denoise(const short* xs, const short* ys, const double* ts, const double* ps, long long n, int H, int W,
                                 double dt, int support, unsigned char* keep, double* ps_out, long long* kept, long long* scratch,
                                 bmc_stream_t stream) {
    BMC_CHECK_ARG(n >= 0 && n < (1ll << 31), "bmc_event_denoise: %lld events are not supported (0 <= n < 2^31)", n);
    BMC_CHECK_ARG(H >= 1 && W >= 1, "bmc_event_denoise: a sensor of %d x %d pixels", H, W);
    BMC_CHECK_ARG(W <= BMC_DENOISE_MAX_W, "bmc_event_denoise: sensors wider than %d pixels are not supported (W = %d)",
                  BMC_DENOISE_MAX_W, W);
    BMC_CHECK_ARG(support >= 1 && support <= 8, "bmc_event_denoise: support %d is outside 1 .. 8", support);
    BMC_CHECK_ARG(isfinite(dt) && dt >= 0.0, "bmc_event_denoise: dt %g is not a finite time >= 0", dt);
    BMC_CHECK_ARG(n == 0 || (xs && ys && ts), "bmc_event_denoise: null event columns");
    BMC_CHECK_ARG(!ps_out || ps || n == 0, "bmc_event_denoise: ps_out needs ps");
    BMC_CHECK_ARG(!kept || scratch, "bmc_event_denoise: the kept count needs scratch");
    BMC_CHECK_ARG(((unsigned long long)scratch & 7ull) == 0, "bmc_event_denoise: scratch is not 8-byte aligned");
    const int R = band_rows(H, W), nb = (H + R - 1) / R;
    if (n > 0) {
        hipLaunchKernelGGL(event_denoise_kernel, dim3(nb), dim3(STEP), 0, (hipStream_t)stream, xs, ys, ts, ps, (int)n, H, W, R, dt,
                           support, keep, ps_out, kept ? scratch : nullptr);
        BMC_CHECK_LAUNCH("bmc_event_denoise");
    }
    if (kept) {
        hipLaunchKernelGGL(event_denoise_finish_kernel, dim3(1), dim3(STEP), 0, (hipStream_t)stream, scratch, n > 0 ? nb : 0, kept);
        BMC_CHECK_LAUNCH("bmc_event_denoise");
    }
    return 0;
}
