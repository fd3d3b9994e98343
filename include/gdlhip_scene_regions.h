/* gdlhip_scene_regions.h -- per-region attributes (zonal statistics) of a label mask for the whole-scene inference of
 * libgdlhip.so: pixel count, bounding box, coordinate sums and the model's confidence of every connected component, reduced on
 * the device from the mask, the labels of gdl_scene_components and the blended canvas of gdlhip_scene.h.  A public header beside
 * gdlhip_scene_sieve.h, gdlhip_scene_rings.h and gdlhip_scene_simplify.h, in the same narrow C dialect: gdlhip/_lib.py binds
 * these symbols from it (SCENE_REGIONS_SIGNATURES) and csrc/scene_regions.hip includes it.  Conventions as in gdlhip.h.
 *
 * A region is a component of gdl_scene_components: one label, the smallest linear index y * W + x of its pixels.  A pixel with
 * label -1 (an ignored one) belongs to no region.  Regions are numbered densely, 0 .. N - 1, by ascending label.
 *
 * Confidence of a pixel, an integer q in 0 .. 65536.  With v the mask value at the pixel and w = canvas[K] the weight sum there,
 * p is the probability of class v: canvas[v] / w for K >= 2; for K == 1, canvas[0] / w when v == 1 and 1 - canvas[0] / w when
 * v == 0.  The quotient is the f32 expression gdl_scene_finish writes to `probs` (one device function, csrc/infer_expr.h), and
 * q = (int) rintf(p * 65536.0f): the scale is a power of two, so the product is exact whether or not 1 - p is fused into it.
 * q = 0 where w == 0 (an uncovered pixel), for every K and v, and q = 0 where the canvas has no plane for v (v >= K for K >= 2,
 * v > 1 for K == 1): no plane out of range is read.  Of the canvas, the two planes canvas[v] and canvas[K] are read at a pixel
 * and no other.
 *
 * Every accumulation is an integer add, minimum or maximum: each result is exact, independent of the order of the adds and the
 * same bits from run to run.  A raster of H * W >= 2^31 pixels is refused (GDL_ERR_INVALID): a linear index is an int32.  No
 * input is modified.  No workgroup waits for another; every dependency is a kernel boundary.  The host learns N between the two
 * calls by one small copy and sizes the second call's arrays by it.
 */
#ifndef GDLHIP_SCENE_REGIONS_H_
#define GDLHIP_SCENE_REGIONS_H_

#include "gdlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* entries per workgroup of the scan: a scan over n entries needs ceil(n / GDL_SCENE_REGIONS_SCAN_TILE) block sums */
#define GDL_SCENE_REGIONS_SCAN_TILE 2048
/* gdl_scene_regions_stats: the edge of the square of pixels one workgroup reduces, the slots of its table in LDS (one label
 * each), and the slots a label is tried at before its run goes to global memory directly */
#define GDL_SCENE_REGIONS_TILE 64
#define GDL_SCENE_REGIONS_TABLE 1024
#define GDL_SCENE_REGIONS_PROBES 8

/* 1. Count.  labels (int32 [H, W]) is what gdl_scene_components gives.  rank[i] (int32 [H * W]) = the number of roots
 * (labels[j] == j) with j < i: at a root, the region's number.  n_regions (one int32 on the device) = N, the number of all.
 * block_sums: int32 [ceil(H * W / GDL_SCENE_REGIONS_SCAN_TILE)] of scratch. */
int gdl_scene_regions_count(const int32_t* labels, int H, int W, int32_t* rank, int32_t* block_sums, int32_t* n_regions,
                            gdl_stream_t stream);

/* 2. Statistics.  mask (uint8 [H, W]) and labels belong together, rank is the count's result and N its n_regions.  canvas: f32
 * [K + 1, H, W] (1 <= K <= 255), or NULL, which skips conf_sum and conf_min (they may then be NULL as well).  Per region, by
 * its number:
 *   label    int32 [N]     the region's label
 *   value    uint8 [N]     the mask value of its pixels
 *   pixels   int32 [N]     their number
 *   bbox     int32 [N, 4]  (x0, y0, x1, y1) in pixel indices, x1 and y1 exclusive
 *   sum_xy   int64 [N, 2]  the sums of the pixels' x and of their y
 *   conf_sum int64 [N]     the sum of q over the pixels
 *   conf_min int32 [N]     the minimum of q over the pixels
 * Two launches.  The first fills the arrays: sums and counts with 0, minima with INT32_MAX, maxima with INT32_MIN.  The second
 * has one workgroup per GDL_SCENE_REGIONS_TILE x GDL_SCENE_REGIONS_TILE pixels: the runs of equal label along a row are reduced
 * inside a wave, the runs' heads accumulate into a table of GDL_SCENE_REGIONS_TABLE labels in LDS (open addressing, at most
 * GDL_SCENE_REGIONS_PROBES slots tried), and every used slot is added to the region's entries with one global atomic per field;
 * a run that finds no slot is added with global atomics of its own.  The atomic traffic of a workgroup is thus proportional to
 * the labels in its tile (up to the table's size), not to its pixels.  A label outside 0 .. H * W - 1 counts as -1, and a rank
 * outside 0 .. N - 1 is not written to, so labels of another mask give wrong numbers but touch nothing outside the arrays.
 * N == 0 launches nothing. */
int gdl_scene_regions_stats(const uint8_t* mask, const int32_t* labels, const int32_t* rank, const float* canvas, int K, int H, int W,
                            int N, int32_t* label, uint8_t* value, int32_t* pixels, int32_t* bbox, int64_t* sum_xy, int64_t* conf_sum,
                            int32_t* conf_min, gdl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GDLHIP_SCENE_REGIONS_H_ */
