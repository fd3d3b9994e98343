/* gdlhip_scene_nodata.h -- nodata for the whole-scene inference of libgdlhip.so: a validity plane of the raster, the count of
 * valid pixels per tile (so that the host can drop the tiles that hold no data before the model sees them), and the cut and the
 * labelling of include/gdlhip_scene.h with that plane.  A public header beside gdlhip_scene.h and gdlhip_scene_tta.h, in the
 * same narrow C dialect: gdlhip/_lib.py binds these symbols from it (SCENE_NODATA_SIGNATURES) and csrc/scene.hip includes it.
 * Conventions as in gdlhip.h.  The blends are untouched: a tile that is dropped is simply not in the list, and a pixel no kept
 * tile covers keeps the weight 0.
 *
 * The plane `valid` is uint8 [H, W], 1 where the raster holds data and 0 where it does not (the kernels that read it take any
 * nonzero value as 1, so an alpha band or a mask from elsewhere can be passed as it is).
 */
#ifndef GDLHIP_SCENE_NODATA_H_
#define GDLHIP_SCENE_NODATA_H_

#include "gdlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* valid[y, x] of a raw raster [C, H, W] of `kind` (GDL_RAW_*) from one nodata value per band, nodata a device float [C].  A
 * sample is nodata when (float)raw == nodata[c]; where nodata[c] is NaN it is nodata when it is NaN (a form for GDL_RAW_F32:
 * no integer sample matches it, and the values live on the device, so it is the caller who refuses it).  rule 0 ("all", the dataset-mask
 * convention): the pixel is invalid when every band is nodata; rule 1 ("any"): when at least one band is.  One pass over the
 * raster, four pixels per thread where W % 4 == 0 and the pointers are aligned for it. */
int gdl_scene_valid(const void* raster, int kind, int C, int H, int W, const float* nodata, int rule, uint8_t* valid,
                    gdl_stream_t stream);

/* counts[t] (int32 [T]) = the number of nonzero valid[y, x] over the part of tile t (th x tw at origins[t], int32 [T][2]) that
 * lies inside the raster; origins may be negative or reach past it as in gdl_scene_cut, and a tile that lies outside
 * altogether counts 0.  One workgroup per tile and one store per tile, no atomics: the counts are exact and reproducible. */
int gdl_scene_tile_valid(const uint8_t* valid, int H, int W, const int32_t* origins, int T, int th, int tw, int32_t* counts,
                         gdl_stream_t stream);

/* gdl_scene_cut (xforms == NULL) or gdl_scene_cut_d4 (xforms != NULL) with one difference: a pixel inside the raster whose
 * valid[y, x] is 0 takes the raw value `fill`, exactly like a position outside the raster, in every band.  The same kernel
 * with one more flag: with a plane of ones the tiles are bit-identical to those of the unmasked calls. */
int gdl_scene_cut_valid(const void* raster, int kind, int C, int H, int W, const uint8_t* valid, const int32_t* origins,
                        const int32_t* xforms, int B, int th, int tw, int fill, float* tiles, int image_min, int image_max,
                        double norm_min, double norm_max, const float* mean, const float* stdv, gdl_stream_t stream);

/* gdl_scene_finish with one difference: where valid[i] == 0 or the weight canvas[K][i] == 0 the mask takes nodata_label
 * (0..255) and every probability is 0; everywhere else the mask and the probabilities are the bits gdl_scene_finish writes.
 * valid may be NULL: then only the pixels no tile covered take nodata_label.  probs may be NULL.  1 <= K <= 255. */
int gdl_scene_finish_valid(const float* canvas, int K, int64_t HW, float threshold, const uint8_t* valid, int nodata_label,
                           uint8_t* mask, float* probs, gdl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GDLHIP_SCENE_NODATA_H_ */
