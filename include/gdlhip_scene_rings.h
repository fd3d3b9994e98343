/* gdlhip_scene_rings.h -- the polygon rings of a label mask for the whole-scene inference of libgdlhip.so: the boundaries of the
 * regions of a uint8 mask as closed rings of lattice points (what GDAL polygonize does to a sieved raster).  A public header
 * beside gdlhip_scene_sieve.h, in the same narrow C dialect: gdlhip/_lib.py binds these symbols from it (SCENE_RINGS_SIGNATURES)
 * and csrc/scene_rings.hip includes it.  Conventions as in gdlhip.h.
 *
 * Lattice: pixel (y, x) is the square with the corners (x, y) and (x + 1, y + 1), x to the right, y down.  A pixel has four
 * sides, travelled with the pixel on the right hand: 0 top (x, y) -> (x+1, y), 1 right (x+1, y) -> (x+1, y+1), 2 bottom
 * (x+1, y+1) -> (x, y+1), 3 left (x, y+1) -> (x, y).  The slot of a side is 4 * (y * W + x) + side, an int32: a raster of
 * H * W >= 2^29 pixels is refused (GDL_ERR_INVALID).
 *
 * A pixel is live when its value is not `ignore_label` (0..255; -1: none) and keep[value] != 0 (keep: 256 uint8 flags on the
 * device).  A side of a live pixel p is a boundary side when the pixel across it lies outside the raster or has another value.
 * The successor of boundary side (p, s), with d_s = E, S, W, N the direction of travel, n_s = N, E, S, W the outward normal,
 * A = p + d_s, B = p + d_s + n_s and same(q) = "q is inside the raster and mask[q] == mask[p]":
 *   connectivity 4:  !same(A) -> (p, (s+1)%4);  else same(B) -> (B, (s+3)%4);  else (A, s)
 *   connectivity 8:   same(B) -> (B, (s+3)%4);  else same(A) -> (A, s);        else (p, (s+1)%4)
 * The successor map is a permutation of the boundary sides and its cycles are the rings.  A ring starts at its smallest slot,
 * rings are ordered by their starts, a corner side is one whose successor has another side number, and vertex k of a ring is
 * the head point of its k-th corner side counted along the successors from the start side (included).  Rings are stored open.
 *
 * The compact index of a boundary side is its rank among all boundary sides in slot order: offsets[p] plus the number of
 * boundary sides of p below it.  The host learns the counts between the calls: n_sides after the first, n_rings and n_vertices
 * after the second, each by one small copy, and sizes the next call's buffers by them.  The mask, H, W, connectivity,
 * ignore_label and keep must be the same in all three.  Integer arithmetic alone: same input, same bits.  No workgroup waits for
 * another; every dependency is a kernel boundary.
 */
#ifndef GDLHIP_SCENE_RINGS_H_
#define GDLHIP_SCENE_RINGS_H_

#include "gdlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* entries per workgroup of the scans: a scan over n entries needs ceil(n / GDL_SCENE_RINGS_SCAN_TILE) block sums */
#define GDL_SCENE_RINGS_SCAN_TILE 2048
/* int32 entries at the end of gdl_scene_rings_trace's `work`: one "changed" flag per doubling round */
#define GDL_SCENE_RINGS_FLAGS 64

/* 1. Count.  offsets[p] (int32 [H * W]) = the number of boundary sides of the pixels before p in row-major order, n_sides
 * (one int32 on the device) = the number of all (E).  bsum: int32 [ceil(H * W / GDL_SCENE_RINGS_SCAN_TILE)] of scratch. */
int gdl_scene_rings_count(const uint8_t* mask, int H, int W, int ignore_label, const uint8_t* keep, int32_t* offsets, int32_t* bsum,
                          int32_t* n_sides, gdl_stream_t stream);

/* 2. Trace.  n_sides is the E the count gave, offsets its result.  Per boundary side, by compact index (int32 [E] each):
 * side_slot its slot, side_next its successor, side_ring the smallest compact index of its ring (the ring's start side), and
 * side_rank the number of corner sides from it (included) to the end of its ring cut open before the start -- at a start side
 * the ring's vertex count.  work: int32 [3 * E + 2 * ceil(E / GDL_SCENE_RINGS_SCAN_TILE) + GDL_SCENE_RINGS_FLAGS]; on return
 * work[e] is the index of the ring that starts at side e and work[E + e] its first vertex (gdl_scene_rings_write reads both).
 * counts (two int32 on the device) = n_rings (R), n_vertices (V).  Both doublings (the minimum for side_ring, the weighted
 * rank for side_rank) run ceil(log2(E)) rounds between ping-pong buffers, a launch per round; a round after one that changed
 * nothing returns at once.  n_sides == 0 launches nothing but the zeroing of counts. */
int gdl_scene_rings_trace(const uint8_t* mask, int H, int W, int connectivity, int ignore_label, const uint8_t* keep,
                          const int32_t* offsets, int n_sides, int32_t* side_slot, int32_t* side_next, int32_t* side_ring,
                          int32_t* side_rank, int32_t* work, int32_t* counts, gdl_stream_t stream);

/* 3. Write.  n_rings and n_vertices are the counts the trace gave, labels (int32 [H, W]) what gdl_scene_components gives for
 * the mask under the same connectivity and ignore_label.  vertices (int32 [V, 2]): (x, y) of every ring's vertices, ring r at
 * ring_offsets[r] .. ring_offsets[r + 1] (int32 [R + 1]); per ring (each [R]) value (uint8) the pixels' class, label (int32)
 * their component, start (int32) the start slot and area2 (int64) the sum of x_i * y_{i+1} - x_{i+1} * y_i over the closed
 * ring: twice the enclosed pixel count for an exterior ring, negative for a hole.  n_sides == 0 writes ring_offsets[0] = 0. */
int gdl_scene_rings_write(const uint8_t* mask, const int32_t* labels, int W, int n_sides, int n_rings, int n_vertices,
                          const int32_t* side_slot, const int32_t* side_next, const int32_t* side_ring, const int32_t* side_rank,
                          const int32_t* work, int32_t* vertices, int32_t* ring_offsets, uint8_t* value, int32_t* label,
                          int32_t* start, int64_t* area2, gdl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GDLHIP_SCENE_RINGS_H_ */
