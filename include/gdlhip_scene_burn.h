/* gdlhip_scene_burn.h -- polygon rings burned into a label raster for the whole-scene inference of libgdlhip.so: the inverse of
 * gdlhip_scene_rings.h (what GDAL rasterize does to a vector layer).  A public header beside gdlhip_scene_rings.h,
 * gdlhip_scene_simplify.h and gdlhip_scene_regions.h, in the same narrow C dialect: gdlhip/_lib.py binds these symbols from it
 * (SCENE_BURN_SIGNATURES) and csrc/scene_burn.hip includes it.  Conventions as in gdlhip.h.
 *
 * Lattice and orientation are those of gdlhip_scene_rings.h: pixel (y, x) is the square (x, y) .. (x + 1, y + 1), y down, and a
 * ring has its region on the right hand (an exterior ring has area2 > 0).  vertices (int32 [V, 2]) are (x, y) in units of
 * 1 / 2^bits pixel, bits in 0 .. 8 (0: the lattice of the traced and simplified rings); ring r is vertices[ring_offsets[r] ..
 * ring_offsets[r + 1]) (int32 [R + 1]), stored open, and burns value[r] (uint8 [R]).  A ring of fewer than 3 vertices
 * contributes nothing.  A coordinate c must satisfy |c| <= 2^20 * 2^bits; vertices may lie outside the raster.
 *
 * The rule, in doubled units with u = 2^bits: a vertex is (2 x, 2 y), the centre of pixel (y, x) is (cx, cy) = ((2 x + 1) u,
 * (2 y + 1) u).  Edge a -> b of a ring (b the cyclic successor of a), dy = by - ay, dx = bx - ax:
 *   - dy == 0 contributes nothing;
 *   - the edge crosses raster row y, 0 <= y < H, iff min(ay, by) <= cy < max(ay, by) (half open: a vertex on a centre line
 *     counts once);
 *   - the crossing column x0 is the smallest integer x with cx >= ax + (cy - ay) dx / dy (a centre exactly on an edge lies
 *     right of it, for every ring alike): x0 = ceil((P - |dy| u) / (2 |dy| u)) with P = sgn(dy) (ax dy + (cy - ay) dx), all
 *     in int64 (magnitudes below 2^62);
 *   - x0 < 0 is clamped to 0, x0 >= W contributes nothing;
 *   - the crossing adds w = +1 (dy < 0: going up, the region to the east) or w = -1 (dy > 0) to C[y, x0] and w * value to
 *     S[y, x0].
 * C and S, summed along each row up to and including x, are the winding number and the value-weighted winding number at the
 * pixel's centre.  The output pixel is S where C == 1 and 0 <= S <= 255; `background` where C == 0 and S == 0; `conflict`
 * everywhere else (overlaps, crossed arcs, reversed rings), and those pixels are counted.
 *
 * Integer adds alone: the result depends on neither the order of the rings nor the order of the atomics, and is the same bits
 * from run to run.  A raster of H * W >= 2^31 pixels is refused (GDL_ERR_INVALID).  No input is modified.  No workgroup waits
 * for another; every dependency is a kernel boundary.  The host learns the number of crossings between the two calls by one
 * small copy.
 */
#ifndef GDLHIP_SCENE_BURN_H_
#define GDLHIP_SCENE_BURN_H_

#include "gdlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* entries per workgroup of the scan: a scan over n entries needs ceil(n / GDL_SCENE_BURN_SCAN_TILE) block sums */
#define GDL_SCENE_BURN_SCAN_TILE 2048
/* the largest `bits`, and the pixels of a row one workgroup of the fill resolves per turn */
#define GDL_SCENE_BURN_BITS_MAX 8
#define GDL_SCENE_BURN_CHUNK 256

/* 1. Count.  Edge e is the one that leaves vertex e.  edge_ring[e] (int32 [V]) = its ring, -1 for a vertex that no ring holds;
 * edge_rows (int32 [V + 1]) = the exclusive scan of the number of raster rows each edge crosses, clipped to 0 .. H: 0 for the
 * edges of a ring of fewer than 3 vertices, for a flat edge and for an edge with a bad entry.  counts (int64 [2] on the device):
 * counts[0] = the number of all crossings, summed in 64 bits (the 32-bit scan wraps silently: the caller refuses a total of
 * 2^31 or more), counts[1] = the number of bad entries: coordinates with |c| > 2^20 * 2^bits, and offsets below their
 * predecessor or outside 0 .. V.  bsum: int32 [ceil((V + 1) / GDL_SCENE_BURN_SCAN_TILE)] of scratch.  vertices and edge_ring
 * may be NULL where n_vertices == 0. */
int gdl_scene_burn_count(const int32_t* vertices, const int32_t* ring_offsets, int n_rings, int n_vertices, int bits, int H, int W,
                         int32_t* edge_ring, int32_t* edge_rows, int32_t* bsum, int64_t* counts, gdl_stream_t stream);

/* 2. Fill.  edge_ring and edge_rows are the count's results, n_cross its counts[0].  plane: int32 [2, H, W] of scratch (C and
 * S), 16-byte aligned, zeroed by the call; out: uint8 [H, W]; reference: uint8 [H, W] or NULL; counts (int64 [2] on the
 * device) = n_conflict, the pixels that are neither a value nor background, and n_differ, the pixels with out != reference
 * (0 without one).  Three kinds of launch: the plane and the counts are zeroed; one thread per crossing finds its edge by a
 * binary search in edge_rows and adds to C and S with int32 atomics (no thread walks an edge); one workgroup per row carries
 * the two prefix sums across chunks of GDL_SCENE_BURN_CHUNK pixels, resolves and counts.  A crossing whose edge, ring or row
 * is not what the rule gives for these vertices (arrays of another call) is dropped: nothing outside the plane is touched.
 * n_cross == 0 or n_rings == 0 writes `background` everywhere (and counts n_differ of that); only out, counts and reference
 * are then looked at. */
int gdl_scene_burn_fill(const int32_t* vertices, const int32_t* ring_offsets, const uint8_t* value, int n_rings, int n_vertices,
                        int bits, int H, int W, const int32_t* edge_ring, const int32_t* edge_rows, int64_t n_cross, int background,
                        int conflict, const uint8_t* reference, int32_t* plane, uint8_t* out, int64_t* counts, gdl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GDLHIP_SCENE_BURN_H_ */
