/* gdlhip_scene_tta.h -- test-time augmentation for the whole-scene inference of libgdlhip.so: the cut and the two blends of
 * include/gdlhip_scene.h with one of the eight symmetries of the square (the dihedral group D4: flips and quarter turns) per
 * tile, applied in the index arithmetic of the gathers.  A public header beside gdlhip_scene.h, in the same narrow C dialect:
 * gdlhip/_lib.py binds these symbols from it (SCENE_TTA_SIGNATURES) and csrc/scene.hip includes it.  Conventions as in
 * gdlhip.h.  The canvas, the weights plane and gdl_scene_finish are those of gdlhip_scene.h: a scene is now a list of
 * (origin, transform) pairs, and a tile may occur in it once per transform.
 *
 * A transform code g is 3 bits: 1 = flip x, 2 = flip y, 4 = transpose.  On the last two dimensions
 *   T_g(x):  y = transpose(x) if g & 4 else x;  y = flip rows of y if g & 2;  y = flip columns of y if g & 1
 * so T_g(x)[i][j] = x[r][c] with (i', j') = (g & 2 ? rows - 1 - i : i, g & 1 ? cols - 1 - j : j) and (r, c) = (j', i') if
 * g & 4, else (i', j').  The inverse of g is g itself when g & 4 == 0 and g with bits 0 and 1 swapped otherwise.  Codes with
 * bit 4 set need th == tw.  xforms is a device array int32 [B], one code per tile; the kernels read xforms[b] & 7, and
 * xforms[b] & 3 when th != tw, so that no value in it can address outside a tile.
 */
#ifndef GDLHIP_SCENE_TTA_H_
#define GDLHIP_SCENE_TTA_H_

#include "gdlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tiles[b] = T_g(the tile gdl_scene_cut cuts at origins[b]) with g = xforms[b]: the same arguments, the same normalisation
 * (one shared device function) and the same `fill` outside the raster, so tiles[b] is bit-identical to the permuted result
 * of gdl_scene_cut.  The tiles are written with 16-byte stores where gdl_scene_cut writes them so; the raster is read
 * element by element. */
int gdl_scene_cut_d4(const void* raster, int kind, int C, int H, int W, const int32_t* origins, const int32_t* xforms, int B, int th,
                     int tw, int fill, float* tiles, int image_min, int image_max, double norm_min, double norm_max,
                     const float* mean, const float* stdv, gdl_stream_t stream);

/* gdl_scene_blend of probabilities probs [B, K, th, tw] f32 that are in the transformed frame (what the model returns for
 * the tile of gdl_scene_cut_d4): canvas pixel p with (dy, dx) = p - origins[t] takes T_g^-1(probs[t])[k][dy][dx], g =
 * xforms[t], with the weight w = wy[dy] * wx[dx] of the canvas frame.  The same fma form, ascending tile order, bounding
 * box and "a pixel no tile covers is not written" as gdl_scene_blend, no atomics: the canvas is bit-identical to
 * gdl_scene_blend of the inverse-permuted probabilities and does not depend on the batching.  1 <= K <= 16. */
int gdl_scene_blend_d4(const float* probs, int B, int K, int th, int tw, const int32_t* origins, const int32_t* xforms, const float* wy,
                       const float* wx, float* canvas, int H, int W, int y0, int y1, int x0, int x1, gdl_stream_t stream);

/* The same from a head's own NHWC f32 map low [B, hi, wi, K] of the transformed tile: the probability is the expression of
 * gdl_scene_blend_lowres (bilinear logits, sigmoid or softmax; shared device functions) evaluated at the position that
 * canvas pixel p has in the transformed tile.  The [B, K, th, tw] probabilities are never written.  1 <= K <= 16. */
int gdl_scene_blend_lowres_d4(const float* low, int B, int hi, int wi, int K, int th, int tw, const int32_t* origins,
                              const int32_t* xforms, const float* wy, const float* wx, float* canvas, int H, int W, int y0, int y1,
                              int x0, int x1, gdl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GDLHIP_SCENE_TTA_H_ */
