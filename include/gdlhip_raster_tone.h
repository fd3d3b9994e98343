/* gdlhip_raster_tone.h -- raster radiometry in front of the whole-scene inference of libgdlhip.so: per-band histograms with
 * nodata left out, quantiles read off them, and a per-band linear stretch with clipping to uint8 or float32 -- what brings a
 * uint16 / int16 / float32 scene into the 8-bit range the served models were trained on, without the raster leaving the device.
 * A public header beside gdlhip_raster.h, in the same narrow C dialect: gdlhip/_lib.py binds these symbols from it
 * (RASTER_TONE_SIGNATURES) and csrc/raster_tone.hip includes it.  Conventions as in gdlhip.h and gdlhip_raster.h: rasters are
 * planar [C, H, W], contiguous, of `kind` (GDL_RAW_*), H * W < 2^31, C <= 65535; nodata: HOST double [C] or NULL (no band has
 * one); has_nodata: HOST uint8 [C] or NULL (every band has one, where nodata is given); a sample is nodata when its band has a
 * nodata value and the sample equals it, and a NaN nodata value means "a NaN sample".  Every refusal (GDL_ERR_INVALID, with a
 * gdl_last_error text) comes before any launch.  The rules below are this library's own; the reference has no counterpart (its
 * inference takes image_min / image_max as given).
 *
 * The histogram.  acc[c][b] += the number of samples of band c that are not nodata and fall in bin b; acc is int64
 * [C, bins + 2], and the two words after the bins count the samples under and over the range.
 *   - GDL_RAW_U8: bins = 256, bin = v.  GDL_RAW_U16: bins = 65536, bin = v.  GDL_RAW_I16: bins = 65536, bin = v + 32768.
 *     `bins` must be given as that number (or 0, which means it); lo and hi must be NULL; the two trailing words stay as they are.
 *   - GDL_RAW_F32: bins in 1..GDL_RASTER_TONE_MAX_BINS and HOST doubles lo[c] < hi[c] per band, finite, with a finite hi - lo.
 *     The bin of a sample v with lo <= v <= hi is min(bins - 1, floor((double(v) - lo) / (hi - lo) * bins)), evaluated in float64
 *     as written: a subtraction, a division by the float64 difference hi - lo, a multiplication, no fused form.  So v == hi goes
 *     to the last bin.  v < lo is counted in word `bins` (under), v > hi in word bins + 1 (over), -inf and +inf among them.  A
 *     NaN sample that is not nodata is counted nowhere.
 *   - Counts are integers added with integer atomics: the result depends on no order and is the same bits from run to run.
 *
 * The quantiles.  For a band with the bin words n[0..bins) (under and over take no part): N = the sum of n, and for a q in
 * [0, 1], r = floor(q * (N - 1)) in float64 (one multiplication), b = the smallest bin whose inclusive cumulative count
 * n[0] + ... + n[b] exceeds r, and the value is origin[c] + b * step[c] in float64 as written (a multiplication, an addition, no
 * fused form).  With (origin, step) = (0, 1) for uint8 and uint16 and (-32768, 1) for int16 that is numpy's
 * quantile(valid samples, q, method="lower"); with (lo, (hi - lo) / bins) for float32 it is the lower edge of the bin that
 * holds that sample, exact to one bin width.  A band with N == 0 gets NaN in every quantile.
 *
 * The stretch.  Per sample v of band c with the bounds (lo, hi) = bounds[c], in float64 as written and without fused forms:
 *     t = (v - lo) / (hi - lo), clamped to [0, 1];  where hi <= lo:  t = v > lo ? 1 : 0;
 *     y = out_lo + t * (out_hi - out_lo);
 *     a GDL_RAW_U8 destination gets floor(y + 0.5) clamped to 0..255, a GDL_RAW_F32 one float(y).
 * A nodata sample, a NaN sample, and every sample of a band whose lo, hi or hi - lo is not finite (the NaN bounds of a band
 * without a valid sample among them) takes dst_nodata, and 0 in the validity plane; every other sample takes 1 there.  There is
 * no gamma: pow is not reproducible bit for bit.
 */
#ifndef GDLHIP_RASTER_TONE_H_
#define GDLHIP_RASTER_TONE_H_

#include "gdlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most bins of a float32 histogram, and the bins of the two 16-bit kinds */
#define GDL_RASTER_TONE_MAX_BINS 65536
/* the most quantiles of one gdl_raster_hist_quantiles call */
#define GDL_RASTER_TONE_MAX_Q 64

/* acc [C, bins + 2] (device int64, 8-byte aligned, zeroed by the caller before the first call; repeated calls add to it) +=
 * the histogram of src [C, H, W] of `kind` as the head of this file says.  lo, hi: HOST double [C] for GDL_RAW_F32, NULL
 * otherwise.  Launches: one per band; a workgroup counts a run of at most 65535 samples in LDS, read once with 16-byte loads
 * where the band's start allows and sample by sample before and after, two 16-bit counters to a word for the 16-bit kinds and
 * float32, and then adds its non-zero counters to acc.  Refused before any launch: a bad kind or extent, null or misaligned
 * pointers, bins that are not the kind's (integer kinds) or outside 1..GDL_RASTER_TONE_MAX_BINS (float32), lo / hi given for
 * an integer kind or missing for float32, a lo[c] >= hi[c], or a lo[c], hi[c] or hi[c] - lo[c] that is not finite. */
int gdl_raster_hist(const void* src, int kind, int C, int H, int W, const double* nodata, const uint8_t* has_nodata, int bins,
                    const double* lo, const double* hi, int64_t* acc, gdl_stream_t stream);

/* out [C, Q] (device float64) = the q[j]-quantiles of every band of acc [C, bins + 2] (what gdl_raster_hist filled) as the head
 * of this file says.  q: HOST double [Q], each in [0, 1], Q in 1..GDL_RASTER_TONE_MAX_Q; origin, step: HOST double [C], finite.
 * Launches: one workgroup per band, an int64 scan over the bins; nothing is copied to the host.  Refused before any launch:
 * C outside 1..65535, bins outside 1..GDL_RASTER_TONE_MAX_BINS, Q outside 1..GDL_RASTER_TONE_MAX_Q, a q[j] outside [0, 1] or
 * NaN, an origin or step that is not finite, null or misaligned pointers. */
int gdl_raster_hist_quantiles(const int64_t* acc, int C, int bins, const double* q, int Q, const double* origin,
                              const double* step, double* out, gdl_stream_t stream);

/* dst [C, H, W] of dst_kind (GDL_RAW_U8 or GDL_RAW_F32) = src [C, H, W] of `kind` stretched band by band from bounds
 * (DEVICE float64 [C, 2]: lo, hi per band, 8-byte aligned; what gdl_raster_hist_quantiles wrote for two quantiles or what
 * the caller uploaded) to out_lo..out_hi as the head of this file says.  valid: uint8 [C, H, W] or NULL.  Launches: one per
 * band, 16 samples per thread with 16-byte loads and stores where the band's start allows, sample by sample before and after.
 * Refused before any launch: a bad kind or extent, a dst_kind that is neither GDL_RAW_U8 nor GDL_RAW_F32, out_lo or out_hi not
 * finite, or outside 0..255 for a GDL_RAW_U8 destination, a dst_nodata the destination cannot hold (GDL_RAW_U8: not an integer
 * in 0..255; GDL_RAW_F32: finite but beyond float32), null or misaligned pointers. */
int gdl_raster_stretch(const void* src, int kind, int C, int H, int W, const double* nodata, const uint8_t* has_nodata,
                       const double* bounds, double out_lo, double out_hi, double dst_nodata, void* dst, int dst_kind,
                       uint8_t* valid, gdl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GDLHIP_RASTER_TONE_H_ */
