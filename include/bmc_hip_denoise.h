/* bmc_hip_denoise.h -- companion of bmc_hip.h: the background-activity (nearest-neighbour correlation) noise filter of a raw
 * event stream, on the GPU.
 *
 * The hot-pixel filter of bmc_hip.h removes stuck pixels; the entry point below removes the other standard defect of a DVS
 * stream, isolated events with no spatio-temporal neighbour (jAER's BackgroundActivityFilter with support 1, its
 * SpatioTemporalCorrelationFilter with support > 1).  It is exported by the same library (csrc/event_denoise.hip) and described,
 * as text made by the compiler from these declarations, by bmc_denoise_abi() -- the records of bmc_abi() (csrc/abi.hip) -- from
 * which bmc_hip/denoise_lib.py builds its binding.  bmc_hip.h itself is unchanged by it.
 *
 * DEFINITION (the contract).  One stream of n events in column order: xs, ys int16, ts float64 (finite and non-decreasing: the
 * caller's to check), ps float64 (optional).  The sensor is H rows x W columns, dt is a finite float64 >= 0 in the units of ts,
 * support an integer k, 1 <= k <= 8.
 *   1. IN RANGE.  Event i is in range iff 0 <= x_i < W and 0 <= y_i < H.  An out-of-range event is never kept, never supports
 *      another event and never touches the surface.
 *   2. SURFACE.  last[y][x] is the index of the latest in-range event at that pixel among the events 0 .. i-1, or none.  Every
 *      in-range event enters the surface, kept or not.  Polarity plays no part; an event with p == 0 is an event like any other.
 *   3. SUPPORT COUNT.  c_i is the number of the eight pixels q around (y_i, x_i) -- not the pixel itself, not a pixel outside the
 *      sensor -- for which j = last[q] exists and ts[i] - ts[j] <= dt: ONE float64 subtraction, rounded once, then compared.
 *      Equal timestamps support each other in column order only: an earlier event supports a later one, never the reverse.
 *   4. RESULT.  keep[i] = in range and c_i >= k, a uint8 0 / 1; ps_out[i] = ps[i] where kept and +0.0 where not (the
 *      recording's polarity column with the noise given weight zero, which every encoder of the library counts as nothing);
 *      kept = the number of ones.
 * The mask is a pure function of the stream: no windows, no dependence on the launch geometry, the same bytes run after run. */
#ifndef BMC_HIP_DENOISE_H
#define BMC_HIP_DENOISE_H

#include "bmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BMC_DENOISE_STEP 256            /* consecutive events a workgroup takes at a time, one per lane */
#define BMC_DENOISE_LDS_WORDS 15360     /* int32 surface entries a workgroup holds: (rows + 2) * (W + 2) of them (60 KB) */
#define BMC_DENOISE_MAX_W 2560          /* the widest sensor: a band is still 3 rows high there */

/* Rows of a band of an H x W sensor: min(H, BMC_DENOISE_LDS_WORDS / (W + 2) - 2); -1 for H or W below 1 or W above
 * BMC_DENOISE_MAX_W.  The launch has ceil(H / rows) workgroups. */
int bmc_event_denoise_band_rows(int H, int W);

/* Bytes of `scratch` bmc_event_denoise needs for an H x W sensor: one int64 partial count per band; -1 where band_rows is. */
long long bmc_event_denoise_scratch_bytes(int H, int W);

/* keep[n] (uint8), ps_out[n] (float64) and kept[0] (int64), all DEVICE memory and each optional (NULL: not written), of the
 * stream xs, ys, ts, ps[n] by the contract above.  ps may be NULL only if ps_out is.  Two launches, no host round trip:
 *   bands   grid ceil(H / rows): a workgroup of BMC_DENOISE_STEP lanes owns `rows` rows of the sensor and keeps the surface of
 *           those rows and of one halo row above and below in LDS, as int32 event indices.  It walks the WHOLE stream in steps of
 *           BMC_DENOISE_STEP consecutive events, lane l taking event base + l: ys is read first, xs only for events in band or
 *           halo.  Per step: the eight neighbours are read from the surface as it stood before the step; after a barrier every
 *           band / halo lane enters its event with an LDS atomicMax; after another barrier the neighbours are read again and a
 *           second read m decides: m < base -- the first read stands; base <= m < i -- m is the answer; m > i -- a later lane hid
 *           what came before, and the lane reads the step's pixel list (LDS) below its own lane for the latest earlier event
 *           at q, the first read standing if there is none.  A band writes keep / ps_out only for the events whose row it
 *           owns (an event whose y is out of range belongs to band 0), so every element is written exactly once, zeros for
 *           out-of-range events included: no memset.  Its kept count goes to scratch[band].
 *   finish  one workgroup adds the band counts (integers) into kept[0]; launched only if kept is given.
 * No global atomics, no workgroup waits for another, the grid is fixed by (H, W).  n == 0 succeeds and writes only the count.
 * scratch: bmc_event_denoise_scratch_bytes(H, W) bytes, 8-byte aligned; may be NULL if kept is.
 * Refused before any launch (-1): n < 0 or n >= 2^31, H or W below 1, W above BMC_DENOISE_MAX_W, support outside 1 .. 8, a dt
 * that is negative or not finite, null xs / ys / ts with n > 0, ps_out without ps, kept without scratch. */
int bmc_event_denoise(const short* xs, const short* ys, const double* ts, const double* ps, long long n, int H, int W, double dt,
                      int support, unsigned char* keep, double* ps_out, long long* kept, long long* scratch, bmc_stream_t stream);

/* The ABI text of this header: fn and const records as bmc_abi() writes them. */
const char* bmc_denoise_abi(void);

#ifdef __cplusplus
}
#endif

#endif /* BMC_HIP_DENOISE_H */
