/* gdlhip_raster.h -- raster preparation in front of the whole-scene inference of libgdlhip.so: a raster put on another raster's
 * grid (what the reference does with rasterio.warp.reproject between two grids of one CRS) and the per-band sums behind the
 * dataset's mean and standard deviation, nodata left out.  A public header beside the gdlhip_scene_*.h ones, in the same narrow
 * C dialect: gdlhip/_lib.py binds these symbols from it (RASTER_SIGNATURES) and csrc/raster.hip includes it.  Conventions as in
 * gdlhip.h.
 *
 * Rasters are planar [C, H, W], contiguous, of `kind` (GDL_RAW_*: uint8, uint16, int16, float32).  Both grids are north-up and
 * in one CRS, so destination pixel (y, x) lies at the source pixel coordinates
 *     u = (x + 0.5) * sx + ox,   v = (y + 0.5) * sy + oy,   sx, sy > 0,
 * each evaluated in float64 as written (one multiplication, one addition, no fused form).  Source sample k of an axis covers
 * [k, k + 1) and has its centre at k + 0.5.
 *
 * The resampling (this header's own rule; it is not GDAL's, and parity with GDAL is not claimed):
 *   - Per axis, with c the centre (u or v), s the scale, n the source size: f = max(1, s), the support is R * f with R = 1
 *     (bilinear: K(t) = max(0, 1 - |t|)) or R = 2 (cubic: Catmull-Rom, a = -0.5: K(t) = 1.5 |t|^3 - 2.5 |t|^2 + 1 below 1,
 *     -0.5 |t|^3 + 2.5 |t|^2 - 4 |t| + 2 below 2).  The taps are k in [max(0, floor(c - R f + 0.5)), min(n, floor(c + R f +
 *     0.5))) with the weight w_k = K((k + 0.5 - c) / f), in float64: the kernel widens where the destination is coarser than the
 *     source (an antialiased resize), and a tap outside the source is simply absent.
 *   - A source sample is masked (m = 0, otherwise 1) when its band has a nodata value and the sample equals it; a NaN nodata
 *     value means "a NaN sample".
 *   - The value is (sum of w_y w_x m v) / (sum of w_y w_x m), both sums in float64 over the taps, one division at the end.
 *   - The pixel is valid iff the source sample that contains (u, v) exists and is not masked, and sum(w m) >=
 *     GDL_RASTER_MIN_VALID_WEIGHT * sum(w), sum(w) = (sum of w_y) * (sum of w_x) over the taps inside the source.  (Cubic
 *     weights are negative in places: without the second condition a masked sum can come arbitrarily close to zero.)  Any other
 *     pixel takes dst_nodata, and 0 in the validity plane.
 *   - Nearest: the sample at (floor(u), floor(v)); dst_nodata where that lies outside the source or is masked.
 *   - A float32 destination gets float(num) / float(den); an integer destination floor(num / den + 0.5) in float64, clamped to
 *     the range of its type (cubic overshoots).  dst_nodata is converted the same way.
 */
#ifndef GDLHIP_RASTER_H_
#define GDLHIP_RASTER_H_

#include "gdlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { GDL_RASTER_NEAREST = 0, GDL_RASTER_BILINEAR = 1, GDL_RASTER_CUBIC = 2 };

/* the share of the taps' weight that must fall on unmasked samples for a pixel to be valid */
#define GDL_RASTER_MIN_VALID_WEIGHT 0.25
/* the largest scale of an axis (destination pixel / source pixel) of bilinear and cubic: at most 4 * 16 + 1 taps per axis */
#define GDL_RASTER_MAX_SCALE 16
/* the blocks per band of the float32 statistics pass (the partial sums of gdl_raster_stats_workspace) */
#define GDL_RASTER_STATS_BLOCKS 1024

/* Bytes of scratch gdl_raster_warp needs for the per-axis tap tables of a destination of Hd x Wd (0 for nearest), or -1 for
 * arguments gdl_raster_warp refuses (gdl_last_error says why).  A host-only query. */
int64_t gdl_raster_warp_workspace(int Hd, int Wd, double sx, double sy, int method);

/* dst [C, Hd, Wd] of dst_kind (`kind`, or GDL_RAW_F32) = src [C, H, W] of `kind` resampled by `method` as the head of this file
 * says.  Replaces the reproject call of geo_deep_learning/utils/rasters.py:68-79 (align_to_reference) for two grids of one CRS.
 * nodata: HOST double [C] or NULL (no band has one); has_nodata: HOST uint8 [C] or NULL (every band has one, where nodata is
 * given).  valid: uint8 [C, Hd, Wd] or NULL.  ws: gdl_raster_warp_workspace() bytes, 8-byte aligned (NULL for nearest).
 * Launches: one thread per destination column and row fills the tap tables (start, count, centre sample, weights and their sum,
 * float64), then per band one thread per destination pixel.  Refused before any launch (GDL_ERR_INVALID): a scale that is not
 * positive and finite, offsets that are not finite, a scale above GDL_RASTER_MAX_SCALE for bilinear and cubic, H * W or Hd * Wd
 * of 2^31 or more, C above 65535, a dst_kind that is neither `kind` nor GDL_RAW_F32. */
int gdl_raster_warp(const void* src, int kind, int C, int H, int W, int Hd, int Wd, double sx, double ox, double sy, double oy,
                    int method, const double* nodata, const uint8_t* has_nodata, double dst_nodata, void* dst, int dst_kind,
                    uint8_t* valid, void* ws, gdl_stream_t stream);

/* Bytes of scratch gdl_raster_stats needs: 0 for the integer kinds, C * GDL_RASTER_STATS_BLOCKS * 3 float64 for GDL_RAW_F32;
 * -1 for arguments it refuses. */
int64_t gdl_raster_stats_workspace(int kind, int C, int H, int W);

/* acc[c] += (the number of samples of band c that are not nodata, their sum, the sum of their squares): the sums behind
 * geo_deep_learning/utils/rasters.py:125-143 (compute_dataset_stats_from_list).  acc: device, 8-byte words [C, 3], zeroed by the
 * caller before the first call; repeated calls add to it.  Word 0 is an int64.  For the integer kinds words 1 and 2 are int64
 * too and exact: a block reduction, then integer atomics, so the result depends on no order (the caller drains the accumulator
 * before 2^63 is reached: 2^30 uint16 samples stay below it).  For GDL_RAW_F32 words 1 and 2 are float64: every block writes its
 * partial sums to ws and a second launch adds them in a fixed order, no floating-point atomics: the same bits from run to run.
 * nodata, has_nodata: HOST arrays as in gdl_raster_warp; a NaN nodata leaves the NaN samples out (unlike the reference, whose
 * `band != nan` leaves nothing out).  H * W of 2^31 or more is refused. */
int gdl_raster_stats(const void* src, int kind, int C, int H, int W, const double* nodata, const uint8_t* has_nodata, int64_t* acc,
                     void* ws, gdl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GDLHIP_RASTER_H_ */
