/* gdlhip_scene_sieve.h -- the sieve of a label mask for the whole-scene inference of libgdlhip.so: the connected components of a
 * uint8 mask and the dissolving of those below a minimum mapping unit into their largest neighbour (what gdal_sieve does to a
 * classified raster before it is vectorised).  A public header beside gdlhip_scene.h, gdlhip_scene_tta.h and
 * gdlhip_scene_nodata.h, in the same narrow C dialect: gdlhip/_lib.py binds these symbols from it (SCENE_SIEVE_SIGNATURES) and
 * csrc/scene_sieve.hip includes it.  Conventions as in gdlhip.h.
 *
 * A component is a maximal set of pixels of one value that is connected under `connectivity` (4: the edge neighbours, 8: the
 * corner neighbours too).  A pixel whose value is `ignore_label` (0..255; -1: none) belongs to no component, connects nothing
 * and is never changed.  Everything below is computed with integer minima, maxima and sums alone, so every result is exact and
 * the same bits from run to run.  A raster of H * W >= 2^31 pixels is refused (GDL_ERR_INVALID): a linear index is an int32.
 */
#ifndef GDLHIP_SCENE_SIEVE_H_
#define GDLHIP_SCENE_SIEVE_H_

#include "gdlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* labels[y, x] (int32 [H, W]) = the smallest linear index y' * W + x' of the pixels of the component of (y, x), -1 on an ignored
 * pixel; sizes[i] (int32 [H * W]) = the number of pixels of the component whose smallest index is i, 0 at every other i.  Three
 * launches: a union-find per 64 x 64 tile in LDS, the unions across the tile edges (agent-scope atomics on the parents, which
 * live in `labels`), and the flattening with the counts.  No workgroup waits for another. */
int gdl_scene_components(const uint8_t* mask, int H, int W, int connectivity, int ignore_label, int32_t* labels, int32_t* sizes,
                         gdl_stream_t stream);

/* One pass of the sieve over `mask` with the labels and sizes gdl_scene_components gave for it (same connectivity and
 * ignore_label).  A component of fewer than min_size pixels is small, every other is kept.  A small component takes the value
 * of the kept component, among those it touches (a pair of pixels adjacent under `connectivity`, one in each), that has the
 * most pixels; of two with equally many, the lower value.  A small component that touches no kept one keeps its value, and so
 * does every kept and every ignored pixel; min_size <= 1 copies the mask.  best (int64 [H * W]) is scratch: at the smallest
 * index of a small component it collects the maximum of (size << 8) | (255 - value) over the kept components it touches.  out
 * (uint8 [H, W]) must not overlap mask. */
int gdl_scene_sieve(const uint8_t* mask, const int32_t* labels, const int32_t* sizes, int H, int W, int connectivity, int min_size,
                    int ignore_label, int64_t* best, uint8_t* out, gdl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GDLHIP_SCENE_SIEVE_H_ */
