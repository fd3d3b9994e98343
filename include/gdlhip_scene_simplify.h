/* gdlhip_scene_simplify.h -- topology-preserving simplification of the polygon rings of gdlhip_scene_rings.h for the whole-scene
 * inference of libgdlhip.so: Douglas-Peucker per arc between junctions, so that two regions that share a boundary get the same
 * simplified boundary, vertex for vertex.  A public header beside gdlhip_scene_rings.h, in the same narrow C dialect:
 * gdlhip/_lib.py binds these symbols from it (SCENE_SIMPLIFY_SIGNATURES) and csrc/scene_simplify.hip includes it.  Conventions
 * as in gdlhip.h.  Lattice, pixel sides, "live" pixel, ignore_label and keep are those of gdlhip_scene_rings.h.
 *
 * Class of a cell: class(q) = mask[q] for a live pixel and 256 for every other cell (outside the raster, equal to ignore_label,
 * or keep[value] == 0).  A unit lattice edge is a boundary edge when the two cells across it have different classes: exactly the
 * edges the rings run along.  A lattice point (x, y), 0 <= x <= W, 0 <= y <= H, is a node when at least 3 of its 4 incident unit
 * lattice edges are boundary edges.  Nodes do not depend on the connectivity; a point where a ring pinches (degree 4) is a node;
 * every other point on a ring has degree 2.
 *
 * Dense ring: a ring of gdl_scene_rings_write lists corners only; the dense ring is that ring with every node that lies strictly
 * inside one of its straight runs inserted at its place (the T-junction seen from the straight side).  Order, orientation and
 * first vertex are unchanged; an inserted node follows the original vertex whose run it lies on.
 *
 * Anchors: the vertices of a dense ring that are nodes.  A ring without any is a free ring (an island, or a hole between exactly
 * two regions); its one anchor is its vertex with the smallest (y, x), y first.  No lattice point occurs twice among the
 * non-anchor vertices of a ring.  The anchors cut the dense ring, taken cyclically, into arcs; a ring with a single anchor is
 * one closed arc from the anchor back to itself.
 *
 * Tolerance: tol_q8 = round(tolerance * 256), 0 <= tolerance <= 2^20 pixels, so 0 <= tol_q8 <= 2^28.
 *
 * Douglas-Peucker on an arc with the end points a and b (lattice points), its interior vertices the candidates.  For a != b the
 * measure of p is c = |(b - a) x (p - a)|, twice the triangle's area and below 2^29 because H * W < 2^29; for a == b (a closed
 * arc, or an arc between two passes of a ring through one pinch) it is |p - a|^2.  The candidate with the largest measure wins,
 * of equal ones the one with the smallest (y, x).  The winner is kept, and splits the arc into two that are treated the same
 * way, iff  c^2 * 2^16 > tol_q8^2 * |b - a|^2  (for a == b:  |p - a|^2 * 2^16 > tol_q8^2), strictly greater, compared in 128
 * bits without any floating point.  Otherwise every interior vertex of the arc is dropped.  This is the distance to the line
 * through a and b, as in the 1973 paper.  Every rule depends on the points alone, never on the direction or the start of the
 * traversal: the two tracings of a shared arc keep the same points.
 *
 * Result: the same R rings in the same order; value, label, start and area2 are not touched (area2 stays the area of the pixel
 * ring).  The output vertices are the kept vertices of each dense ring in dense order; anchors are always kept, inserted nodes
 * included.  A ring may come out with fewer than 3 vertices: it collapsed, which is no error.
 *
 * The host learns the counts between the calls, each by one small copy: the dense vertex count D after the count, the "changed"
 * flag after every group of rounds, the output vertex count after the write.  Integer arithmetic and integer max / min atomics
 * alone: same input, same bits.  No thread walks a ring or an arc, no workgroup waits for another, every dependency is a kernel
 * boundary.  No input is modified.  Vertices outside the lattice or runs that are not axis-parallel (rings of another mask)
 * insert nothing and read nothing outside the node plane.
 */
#ifndef GDLHIP_SCENE_SIMPLIFY_H_
#define GDLHIP_SCENE_SIMPLIFY_H_

#include "gdlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* entries per workgroup of the scans: a scan over n entries needs ceil(n / GDL_SCENE_SIMPLIFY_SCAN_TILE) block sums */
#define GDL_SCENE_SIMPLIFY_SCAN_TILE 2048
/* the rounds of one gdl_scene_simplify_rounds call at the most, and what the host launches between two reads of `changed` */
#define GDL_SCENE_SIMPLIFY_ROUNDS 8

/* 1. Nodes.  nodes (uint8 [(H + 1), (W + 1)]): 1 at a node, 0 elsewhere.  H * W >= 2^29 is refused as by the rings. */
int gdl_scene_nodes(const uint8_t* mask, int H, int W, int ignore_label, const uint8_t* keep, uint8_t* nodes, gdl_stream_t stream);

/* 2. Count.  vertices (int32 [V, 2]) and ring_offsets (int32 [R + 1]) are what gdl_scene_rings_write gave.  pos (int32 [V + 1]):
 * pos[i] = the dense index of ring vertex i, i.e. i plus the nodes strictly inside the runs that start before it; pos[V] = D, also
 * written to n_dense (one int32 on the device).  bsum: int32 [ceil((V + 1) / GDL_SCENE_SIMPLIFY_SCAN_TILE)] of scratch.
 * n_rings == 0 or n_vertices == 0 launches nothing but the zeroing of n_dense. */
int gdl_scene_simplify_count(const uint8_t* nodes, int H, int W, const int32_t* vertices, const int32_t* ring_offsets, int n_rings,
                             int n_vertices, int32_t* pos, int32_t* bsum, int32_t* n_dense, gdl_stream_t stream);

/* 3. Dense rings and arcs.  n_dense is the D the count gave, pos its result.  dense (int32 [D, 2]): the vertices of the dense
 * rings, ring r at dense_offsets[r] .. dense_offsets[r + 1] (int32 [R + 1]).  kept (uint8 [D]): 1 at every anchor (the free
 * rings' included), 0 elsewhere.  seg (int32 [4 * D + GDL_SCENE_SIMPLIFY_ROUNDS]) and key (int64 [D]) are the state of the
 * rounds: seg[k] and seg[D + k] are the dense indices of the two end points of the segment that candidate k lies in (an arc at
 * first; -1: k is no candidate any more), seg[2 * D + k], seg[3 * D + k] and key[k] the arg-max slots of the segment that starts
 * at k, the last entries of seg the flags of the rounds.  work: int32 [2 * R + 2 * D + 1 + ceil((D + 1) /
 * GDL_SCENE_SIMPLIFY_SCAN_TILE)] of scratch, 8-byte aligned. */
int gdl_scene_simplify_dense(const uint8_t* nodes, int H, int W, const int32_t* vertices, const int32_t* ring_offsets, int n_rings,
                             int n_vertices, const int32_t* pos, int n_dense, int32_t* dense, int32_t* dense_offsets, uint8_t* kept,
                             int32_t* seg, int64_t* key, int32_t* work, gdl_stream_t stream);

/* 4. Rounds.  One round splits every current segment once: the arg-max of the measure over its candidates (launch 1: a 64-bit
 * atomic max at the slot of the segment's first end point, measure and inverted lattice index y * (W + 1) + x packed into one
 * word for a != b; for a == b, which only round 0 of the first call can meet, the measure alone and a second launch with an
 * atomic min of the lattice index), the test of the winner, which marks it in `kept` (launch 2), and every candidate's new
 * segment from the winner's index (launch 3).  first != 0: this is the first call after gdl_scene_simplify_dense.  n_rounds in
 * 1 .. GDL_SCENE_SIMPLIFY_ROUNDS.  changed (one int32 on the device) = 1 when the last round kept a vertex, so that another
 * call is needed, else 0; a round after one that kept none returns at once.  The depth of Douglas-Peucker depends on the data
 * (up to the length of an arc), so the host repeats the call until changed == 0. */
int gdl_scene_simplify_rounds(const int32_t* dense, int W, int n_dense, int tol_q8, int first, int n_rounds, uint8_t* kept,
                              int32_t* seg, int64_t* key, int32_t* changed, gdl_stream_t stream);

/* 5. Write.  Compacts the kept vertices: out_vertices (int32 [D, 2], the first n_out rows written), out_offsets (int32 [R + 1]),
 * n_out (one int32 on the device).  scan: int32 [D + 1 + ceil((D + 1) / GDL_SCENE_SIMPLIFY_SCAN_TILE)] of scratch.
 * n_rings == 0 or n_dense == 0 writes out_offsets[0 .. R] = 0 and n_out = 0. */
int gdl_scene_simplify_write(const int32_t* dense, const int32_t* dense_offsets, int n_rings, int n_dense, const uint8_t* kept,
                             int32_t* scan, int32_t* out_vertices, int32_t* out_offsets, int32_t* n_out, gdl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GDLHIP_SCENE_SIMPLIFY_H_ */
