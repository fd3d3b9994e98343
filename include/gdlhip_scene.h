/* gdlhip_scene.h -- whole-scene inference of libgdlhip.so: cutting normalised tiles out of a raster, stitching the tiles'
 * class probabilities into one weighted canvas, and labelling the canvas.  A public header beside include/gdlhip.h (which it
 * includes for gdl_stream_t, the GDL_RAW_* kinds and the gdl_status values) and written in the same narrow C dialect:
 * gdlhip/_lib.py binds these symbols from it (SCENE_SIGNATURES) with the parser that reads the main header, and
 * csrc/scene.hip includes it, so the compiler checks every definition against it.  Conventions as in gdlhip.h: device
 * pointers owned by the caller, every call enqueues on the caller's stream and returns 0 or a negative gdl_status.
 *
 * One scene is: a raster [C, H, W]; a list of tile origins (y0, x0) from the host planner (gdlhip/scene.py: plan_tiles), fed
 * in batches of B tiles as a device array int32 [B][2]; a canvas [K+1, H, W] f32 that starts at zero, whose planes 0..K-1
 * hold the window-weighted sums of the class probabilities and whose plane K holds the sum of the weights.
 */
#ifndef GDLHIP_SCENE_H_
#define GDLHIP_SCENE_H_

#include "gdlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tiles[b, c, dy, dx] = normalise(raster[c, origins[b][0] + dy, origins[b][1] + dx]) for B tiles of th x tw: raster is a raw
 * [C, H, W] image of `kind` (GDL_RAW_*), tiles is NCHW f32 [B, C, th, tw].  An origin may be negative or reach past the
 * raster: a position outside it takes the raw value `fill` before it is normalised.  The normalisation is the expression of
 * gdl_normalize_range, one shared device function with the same rounding order and the same scalar arguments, so a tile that
 * lies inside the raster is bit-identical to gdl_normalize_range of the sliced tile.  image_max == image_min is an error (-1,
 * with the message of gdl_normalize_range). */
int gdl_scene_cut(const void* raster, int kind, int C, int H, int W, const int32_t* origins, int B, int th, int tw, int fill,
                  float* tiles, int image_min, int image_max, double norm_min, double norm_max, const float* mean,
                  const float* stdv, gdl_stream_t stream);

/* Blended stitching of full-resolution probabilities probs [B, K, th, tw] f32 into canvas [K+1, H, W] f32.  For every canvas
 * pixel p = (y, x) with y0 <= y < y1 and x0 <= x < x1 (the batch's bounding box, clipped to the canvas) and every tile t of
 * the batch that covers it, in ascending t, with (dy, dx) = p - origins[t] and w = wy[dy] * wx[dx] (wy [th] and wx [tw] f32):
 *   canvas[k][p] = fma(w, probs[t][k][dy][dx], canvas[k][p]) for k < K, and canvas[K][p] += w.
 * A gather: one thread owns a canvas pixel and walks the tiles that cover it, with the canvas value as the running sum and
 * no atomics, so the result does not depend on how the tile list is split into batches as long as the tiles keep their
 * order.  A pixel that no tile of the batch covers is neither read back nor written; the parts of a tile outside the canvas
 * are ignored.  1 <= K <= 16. */
int gdl_scene_blend(const float* probs, int B, int K, int th, int tw, const int32_t* origins, const float* wy, const float* wx,
                    float* canvas, int H, int W, int y0, int y1, int x0, int x1, gdl_stream_t stream);

/* The same accumulation straight from a head's own NHWC f32 map low [B, hi, wi, K] with the target size th x tw: the
 * probability of tile pixel (dy, dx) is evaluated on the fly with the expression of gdl_upsample_probs (bilinear logits,
 * align_corners = false; sigmoid for K == 1, softmax with max-subtraction for 2 <= K <= 16; shared device functions), so the
 * [B, K, th, tw] probabilities are never written.  Any other K is an error (-1). */
int gdl_scene_blend_lowres(const float* low, int B, int hi, int wi, int K, int th, int tw, const int32_t* origins, const float* wy,
                           const float* wx, float* canvas, int H, int W, int y0, int y1, int x0, int x1, gdl_stream_t stream);

/* Labels of a finished canvas [K+1, HW] f32 -> mask [HW] uint8 and, when probs is not NULL, probs [K, HW] f32 =
 * canvas[k] / canvas[K].  K >= 2: mask = arg-max over canvas[k] (no division; the lowest index wins a tie).  K == 1: mask =
 * canvas[0] / canvas[1] > threshold, evaluated in f32.  A pixel whose weight sum canvas[K] is 0 (never covered) gets mask 0
 * and probabilities 0.  1 <= K <= 255. */
int gdl_scene_finish(const float* canvas, int K, int64_t HW, float threshold, uint8_t* mask, float* probs, gdl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GDLHIP_SCENE_H_ */
