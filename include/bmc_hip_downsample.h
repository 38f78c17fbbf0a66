/* bmc_hip_downsample.h -- companion of bmc_hip.h: the LR event stream of an HR-only recording, by integrate-and-fire over blocks
 * of s x s HR pixels, on the GPU.
 *
 * Every training and evaluation entry point takes a recording as a pair of streams (lr, gt).  The entry points below make the LR
 * half from the HR one: an LR pixel sees the mean brightness change of its block and fires when the HR steps of one sign, net
 * of the other, reach the count that equals one LR contrast step -- the DVS pixel model applied to the block, with hysteresis.
 * They are exported by the same library (csrc/event_downsample.hip) and described, as text made by the compiler from these
 * declarations, by bmc_downsample_abi() -- the records of bmc_abi() (csrc/abi.hip) -- from which bmc_hip/downsample_lib.py builds
 * its binding.  bmc_hip.h itself is unchanged by it.
 *
 * DEFINITION (the contract).  One stream of n events in column order: xs, ys int16, ts float64 (non-decreasing: the caller's
 * business; the result depends on column order only), ps float64.  The HR sensor is H rows x W columns, s an integer scale,
 * 1 <= s <= 16, T an integer threshold, 1 <= T <= 32767.  The LR sensor is h x w = ceil(H / s) x ceil(W / s); edge LR pixels
 * cover fewer HR pixels and keep the same T.
 *   1. COUNTED.  Event i is counted iff 0 <= x_i < W, 0 <= y_i < H and p_i > 0 or p_i < 0; its step is +1 or -1.  Any other
 *      event (p == +-0.0, which is how the noise filter marks a drop; a NaN polarity; an out-of-range event) touches nothing.
 *   2. ACCUMULATOR.  Each LR pixel (y_i / s, x_i / s) (integer division) has an int accumulator a that starts at 0.  Counted
 *      events act on it in column order, equal timestamps included: a += step; if a == T the event FIRES +1 and a = 0; if
 *      a == -T it FIRES -1 and a = 0.
 *   3. OUTPUT.  The firing events in column order of the input.  Output event k, from input event i: xs = x_i / s, ys = y_i / s
 *      (int16), ts = ts[i] (the same bits), ps = +1.0 or -1.0 (float64).  count (int64, DEVICE memory) is their number.
 *   4. CAPACITY.  A pixel needs at least T counted events per fire, so count <= n / T (integer division): the capacity of the
 *      output columns, exact, never exceeded, reachable.  Nothing is sized by a host round trip.
 * The result is a pure function of the stream and (H, W, s, T): the same bytes run after run, whatever the launch geometry.
 *
 * FOUR STAGES, none of which walks the whole stream once per tile of the sensor:
 *   keys    bmc_event_downsample_keys, one launch: one lane per event.
 *   group   the caller's: ONE stable ascending sort of keys[n] -> sorted keys and the permutation (int64 original indices), so
 *           that every LR pixel's events are contiguous and in column order (torch.sort(stable=True) in bmc_hip.encodings).
 *   walk    bmc_event_downsample_walk, one launch: one lane per LR pixel.
 *   gather  bmc_event_downsample_gather, two launches: the ordered stream compaction of fire[n] into the output columns.
 * BMC_DOWNSAMPLE_LAUNCHES = 4 launches of this library per stream with n > 0 (n == 0: the two of the gather, which write
 * count = 0), no memset, no global atomics, no workgroup waits for another. */
#ifndef BMC_HIP_DOWNSAMPLE_H
#define BMC_HIP_DOWNSAMPLE_H

#include "bmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BMC_DOWNSAMPLE_MAX_SCALE 16
#define BMC_DOWNSAMPLE_MAX_THRESHOLD 32767
#define BMC_DOWNSAMPLE_LANES 256        /* lanes of every workgroup: events of a keys workgroup, LR pixels of a walk workgroup */
#define BMC_DOWNSAMPLE_TILE 1024        /* events a gather workgroup takes at a time: 4 rounds of one event per lane */
#define BMC_DOWNSAMPLE_MAX_PARTS 2048   /* the most workgroups (chunks) of a gather launch */
#define BMC_DOWNSAMPLE_LAUNCHES 4       /* keys, walk, gather (totals), gather (write) */

/* n / T, the capacity of the output columns (rule 4); -1 for n < 0, n >= 2^31 or T outside 1 .. BMC_DOWNSAMPLE_MAX_THRESHOLD. */
long long bmc_event_downsample_capacity(long long n, int T);

/* Events of a gather chunk for a stream of n: the smallest multiple of BMC_DOWNSAMPLE_TILE with at most
 * BMC_DOWNSAMPLE_MAX_PARTS chunks, ceil(ceil(max(n, 1) / BMC_DOWNSAMPLE_MAX_PARTS) / TILE) * TILE; the launches have
 * max(1, ceil(n / chunk)) workgroups.  -1 for n < 0 or n >= 2^31. */
long long bmc_event_downsample_chunk(long long n);

/* Bytes of `scratch` bmc_event_downsample_gather needs for a stream of n: one uint32 total per chunk, rounded up to a multiple
 * of 8; -1 where the chunk is. */
long long bmc_event_downsample_scratch_bytes(long long n);

/* keys[n] (int32) and fire[n] (int8), DEVICE memory, of the stream xs, ys, ps[n].  One launch, grid ceil(n / LANES), lane l of
 * workgroup g takes event g * LANES + l: keys[i] = (y_i / s) * w + x_i / s for a counted event (rule 1), the sentinel h * w for
 * any other; fire[i] = 0 -- this launch is the zero fill of fire.  n == 0: no launch.
 * Refused before any launch (-1): n < 0 or n >= 2^31, H or W below 1, s outside 1 .. BMC_DOWNSAMPLE_MAX_SCALE, h * w not below
 * 2^31 - 1, null xs / ys / ps / keys / fire with n > 0. */
int bmc_event_downsample_keys(const short* xs, const short* ys, const double* ps, long long n, int H, int W, int s, int* keys,
                              signed char* fire, bmc_stream_t stream);

/* fire[n] of rule 2 from sorted[n] (int32: keys in ascending order) and perm[n] (int64: sorted[j] == keys[perm[j]], equal keys in
 * rising perm -- a stable sort).  One launch, grid ceil(h * w / LANES), one lane per LR pixel q: it finds its segment
 * [lower_bound(q), lower_bound(q + 1)) of sorted by binary search, walks it in order with the accumulator in a register (the step
 * is the sign of ps[perm[j]]) and writes fire[perm[j]] = +1 / -1 at the ORIGINAL index of each firing event.  Every other element
 * of fire keeps the zero of the keys launch; the sentinel's segment belongs to no lane.  An entry of perm outside 0 .. n-1 is
 * skipped, not followed.  No LDS, no barrier, no atomic.  n == 0: no launch.
 * Refused before any launch (-1): as the keys, T outside 1 .. BMC_DOWNSAMPLE_MAX_THRESHOLD, null sorted / perm / ps / fire with
 * n > 0. */
int bmc_event_downsample_walk(const int* sorted, const long long* perm, const double* ps, long long n, int H, int W, int s, int T,
                              signed char* fire, bmc_stream_t stream);

/* The output columns of rule 3 from fire[n]: out_xs, out_ys (int16), out_ts, out_ps (float64) of `capacity` entries each and
 * count[0] (int64), DEVICE memory.  Entries at count and after are not written; an output position at or above capacity is
 * dropped (by rule 4 there is none for capacity >= n / T).  Two launches of grid max(1, ceil(n / chunk)), no host round trip:
 *   totals  workgroup c counts the firing events of its chunk [c * chunk, min(n, (c + 1) * chunk)) -> scratch[c] (uint32);
 *   write   workgroup c adds the totals of the chunks before it (workgroup 0 adds all of them and writes count[0]), then takes
 *           its chunk BMC_DOWNSAMPLE_TILE events at a time: each wave ranks its firing lanes by ballot and popcount, one LDS
 *           exchange orders the waves and rounds, the firing events' indices go to LDS at their rank, and lane p stores output
 *           p of the tile: consecutive lanes store consecutive outputs.
 * No global atomics, no workgroup waits for another.  n == 0 succeeds and writes count[0] = 0.
 * Refused before any launch (-1): n < 0 or n >= 2^31, s outside its range, capacity < 0, null count or scratch, null xs / ys /
 * ts / fire with n > 0, a null output column with capacity > 0, a scratch that is not 8-byte aligned. */
int bmc_event_downsample_gather(const short* xs, const short* ys, const double* ts, const signed char* fire, long long n, int s,
                                short* out_xs, short* out_ys, double* out_ts, double* out_ps, long long capacity, long long* count,
                                unsigned* scratch, bmc_stream_t stream);

/* The ABI text of this header: fn and const records as bmc_abi() writes them. */
const char* bmc_downsample_abi(void);

#ifdef __cplusplus
}
#endif

#endif /* BMC_HIP_DOWNSAMPLE_H */
