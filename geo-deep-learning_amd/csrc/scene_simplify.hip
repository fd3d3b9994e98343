// Simplification of the polygon rings (include/gdlhip_scene_simplify.h): Douglas-Peucker per arc between the nodes of the
// boundary graph.  Definitions (class, node, dense ring, anchor, arc, measure, tie rule, test) are the header's.
//
// Everything is one thread per vertex (of the rings, then of the dense rings); a thread never walks a ring or an arc.  The only
// loops are the binary search of a vertex's ring in the ring offsets and the sweep of one straight run of a ring for the nodes
// inside it (all runs together are as long as the rings have sides).  The launches, each seeing the stores of the one before
// through the kernel boundary (V ring vertices, D dense vertices, R rings):
//   nodes    simplify_nodes       per lattice point: the classes of its four cells -> degree >= 3
//   count    simplify_count       per ring vertex: 1 + the nodes strictly inside its run; exclusive scan over V + 1 -> pos, D
//   dense    simplify_dense       per ring vertex: the corner and the inserted nodes at pos[i] ..; the anchor flag of each
//            simplify_offsets     per ring: dense_offsets[r] = pos[ring_offsets[r]]
//            scan over D + 1      the anchors before every dense vertex (A)
//            simplify_free_min    per dense vertex of a ring without anchors: atomic min of (lattice index, k) at the ring
//            simplify_arcs        per dense vertex: the anchor list is alist[A[k]] = k; a candidate's arc is (the anchor
//                                 before it, the anchor after it), cyclically inside its ring's range of A
//   rounds   simplify_argmax      per candidate: 64-bit atomic max of its key at the slot of its segment's first end point
//            simplify_closed_min  (round 0 of the first call) a == b: atomic min of the lattice index among the largest
//            simplify_test        the candidate whose key stands in the slot is the winner: the 128-bit test; kept, win
//            simplify_split       per candidate: dead when its segment kept nothing, else the half on its side of the winner
//   write    simplify_flags, scan over D + 1, simplify_scatter
// Segments are pairs of dense indices (lo, hi), travelled from lo to hi along the ring; the last arc of a ring wraps around the
// ring's end, which shows as lo >= hi.  Whether a candidate lies before the winner is decided by ord(v) = v, plus 2^32 where
// v < lo: that needs no ring, and it stays right for every sub-segment, whose lo is either the old one or the winner.
// Integer max / min atomics are order-independent, so the bits do not depend on scheduling.  Every index that a kernel reads
// from memory and then uses as an address is held against the array's size first: the arrays are the caller's.
#include "gdl_common.h"
#include "../../include/gdlhip_scene_simplify.h"

namespace {

#include "scan_u32.h"
#include "scene_common.h"
static_assert(SCAN_TILE == GDL_SCENE_SIMPLIFY_SCAN_TILE, "the header states the scan's block size for the callers' scratch");

typedef unsigned long long u64;

// ------------------------------------------------------------------ 1. nodes
// the class of cell (y, x): the value of a live pixel (Raster, scene_common.h), 256 for every other cell
__device__ __forceinline__ int cell_class(const Raster& r, int y, int x) {
  const int v = r.cell(y, x);
  return v < 0 ? 256 : v;
}

__global__ __launch_bounds__(256) void simplify_nodes_kernel(Raster r, uint8_t* __restrict__ nodes) {
  const int64_t n = (int64_t)(r.H + 1) * (r.W + 1);
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
    const int y = (int)(q / (r.W + 1)), x = (int)(q % (r.W + 1));
    const int nw = cell_class(r, y - 1, x - 1), ne = cell_class(r, y - 1, x), sw = cell_class(r, y, x - 1), se = cell_class(r, y, x);
    nodes[q] = (nw != ne) + (sw != se) + (nw != sw) + (ne != se) >= 3;
  }
}

// ------------------------------------------------------------------ 2. count, 3. dense rings and arcs
// the largest r in 0 .. R - 1 with offsets[r] <= i (R >= 1); ends whatever the array holds
__device__ __forceinline__ int ring_of(const int32_t* __restrict__ offsets, int R, int i) {
  int lo = 0, hi = R - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The run that starts at ring vertex i: its first point, its unit step and its length in steps.  len == 0 where there is
// nothing to sweep: a point outside the lattice or a run that is not axis-parallel, which the rings of this mask never have.
struct Run {
  int x, y, dx, dy, len;
  bool first_in_lattice;
};

__device__ __forceinline__ Run run_of(const int2* __restrict__ vertices, const int32_t* __restrict__ ring_offsets, int R, int V, int H, int W,
                                      int i) {
  const int r = ring_of(ring_offsets, R, i);
  const int end = ring_offsets[r + 1];
  int next = i + 1 < end ? i + 1 : ring_offsets[r];
  if (!in_range(next, V)) next = i;
  const int2 p = vertices[i], q = vertices[next];
  Run run{p.x, p.y, 0, 0, 0, p.x >= 0 && p.x <= W && p.y >= 0 && p.y <= H};
  if (!run.first_in_lattice || q.x < 0 || q.x > W || q.y < 0 || q.y > H) return run;
  if (p.y == q.y) { run.dx = q.x > p.x ? 1 : -1; run.len = abs(q.x - p.x); }
  else if (p.x == q.x) { run.dy = q.y > p.y ? 1 : -1; run.len = abs(q.y - p.y); }
  return run;
}

__global__ __launch_bounds__(256) void simplify_count_kernel(const uint8_t* __restrict__ nodes, int H, int W, const int2* __restrict__ vertices,
                                                             const int32_t* __restrict__ ring_offsets, int R, int V,
                                                             uint32_t* __restrict__ pos) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // the grid covers V + 1
  if (i > V) return;
  uint32_t n = 0;
  if (i < V) {
    const Run run = run_of(vertices, ring_offsets, R, V, H, W, (int)i);
    const int64_t at = (int64_t)run.y * (W + 1) + run.x, step = (int64_t)run.dy * (W + 1) + run.dx;
    n = 1;
    for (int t = 1; t < run.len; ++t) n += nodes[at + t * step] != 0;
  }
  pos[i] = n;
}

__global__ __launch_bounds__(256) void simplify_dense_kernel(const uint8_t* __restrict__ nodes, int H, int W, const int2* __restrict__ vertices,
                                                             const int32_t* __restrict__ ring_offsets, int R, int V,
                                                             const int32_t* __restrict__ pos, int D, int2* __restrict__ dense,
                                                             uint8_t* __restrict__ kept, uint32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= V) return;
  if (i == 0) flags[D] = 0;      // the scan runs over D + 1 entries, so that A[D] is the number of all anchors
  const Run run = run_of(vertices, ring_offsets, R, V, H, W, (int)i);
  const int64_t at = (int64_t)run.y * (W + 1) + run.x, step = (int64_t)run.dy * (W + 1) + run.dx;
  int k = pos[i];
  if (in_range(k, D)) {
    const bool node = run.first_in_lattice && nodes[at] != 0;
    dense[k] = make_int2(run.x, run.y);
    kept[k] = node;
    flags[k] = node;
  }
  for (int t = 1; t < run.len; ++t) {
    if (nodes[at + t * step] == 0) continue;
    ++k;
    if (in_range(k, D)) {
      dense[k] = make_int2(run.x + t * run.dx, run.y + t * run.dy);
      kept[k] = 1;
      flags[k] = 1;
    }
  }
}

__global__ __launch_bounds__(256) void simplify_offsets_kernel(const int32_t* __restrict__ ring_offsets, int R, int V,
                                                               const int32_t* __restrict__ pos, int D, int32_t* __restrict__ dense_offsets) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > R) return;
  const int o = ring_offsets[r];
  const int d = (unsigned)o <= (unsigned)V ? pos[o] : D;
  dense_offsets[r] = (unsigned)d <= (unsigned)D ? d : D;
}

__device__ __forceinline__ uint32_t lattice_index(int2 p, int W) { return (uint32_t)((int64_t)p.y * (W + 1) + p.x); }

// the ring of dense vertex k and the range of the anchor counts A that belongs to it; false where the offsets are not a ring's
__device__ __forceinline__ bool anchors_of_ring(const int32_t* __restrict__ dense_offsets, int R, int D, const uint32_t* __restrict__ A, int k,
                                                int& r, uint32_t& first, uint32_t& last) {
  r = ring_of(dense_offsets, R, k);
  const int s = dense_offsets[r], e = dense_offsets[r + 1];
  if ((unsigned)s > (unsigned)D || (unsigned)e > (unsigned)D) return false;
  first = A[s];
  last = A[e];
  return true;
}

__global__ __launch_bounds__(256) void simplify_free_min_kernel(const int2* __restrict__ dense, const int32_t* __restrict__ dense_offsets, int R,
                                                                int D, int W, const uint32_t* __restrict__ A, u64* ring_min) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= D) return;
  int r;
  uint32_t first, last;
  if (!anchors_of_ring(dense_offsets, R, D, A, (int)k, r, first, last) || first != last) return;
  __hip_atomic_fetch_min(ring_min + r, (u64)lattice_index(dense[k], W) << 32 | (u64)k, RLX_AGENT);
}

__global__ __launch_bounds__(256) void simplify_anchor_list_kernel(int D, const uint8_t* __restrict__ kept, const uint32_t* __restrict__ A,
                                                                   int32_t* __restrict__ alist) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= D) return;
  if (kept[k] && in_range((int)A[k], D)) alist[A[k]] = (int)k;
}

__global__ __launch_bounds__(256) void simplify_arcs_kernel(const int32_t* __restrict__ dense_offsets, int R, int D,
                                                            const uint32_t* __restrict__ A, const int32_t* __restrict__ alist,
                                                            const u64* __restrict__ ring_min, uint8_t* __restrict__ kept,
                                                            int32_t* __restrict__ seg, u64* __restrict__ key) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= D) return;
  int r, lo = -1, hi = -1;
  uint32_t first, last;
  if (anchors_of_ring(dense_offsets, R, D, A, (int)k, r, first, last)) {
    if (first == last) {      // a free ring: one closed arc from its smallest vertex
      const int w = (int)(uint32_t)ring_min[r];
      if (w == k) kept[k] = 1;
      else if (in_range(w, D)) lo = hi = w;
    } else if (!kept[k]) {
      const uint32_t c = A[k];      // first <= c <= last
      const uint32_t before = c > first ? c - 1 : last - 1, after = c < last ? c : first;
      if (in_range((int)before, D) && in_range((int)after, D)) {
        lo = alist[before];
        hi = alist[after];
        if (!in_range(lo, D) || !in_range(hi, D)) lo = hi = -1;
      }
    }
  }
  seg[k] = lo;
  seg[(int64_t)D + k] = hi;
  seg[2 * (int64_t)D + k] = -1;
  seg[3 * (int64_t)D + k] = -1;      // all ones: the start of the closed arcs' atomic min
  key[k] = 0;
}

// ------------------------------------------------------------------ 4. rounds
struct Candidate {
  int lo;              // the slot of its segment; -1: no candidate
  bool closed;         // a == b
  u64 measure, d2;     // c or |p - a|^2; |b - a|^2
  uint32_t index;      // y * (W + 1) + x
  __device__ __forceinline__ u64 packed() const { return measure << 32 | (uint32_t)~index; }      // a != b: c < 2^29
};

__device__ __forceinline__ Candidate candidate(const int2* __restrict__ dense, const int32_t* __restrict__ seg, int D, int W, int64_t k) {
  Candidate c{-1, false, 0, 0, 0};
  if (k >= D) return c;
  const int lo = seg[k], hi = seg[(int64_t)D + k];
  if (!in_range(lo, D) || !in_range(hi, D)) return c;
  const int2 a = dense[lo], b = dense[hi], p = dense[k];
  const int64_t bx = (int64_t)b.x - a.x, by = (int64_t)b.y - a.y, px = (int64_t)p.x - a.x, py = (int64_t)p.y - a.y;
  c.lo = lo;
  c.closed = bx == 0 && by == 0;
  const int64_t cross = bx * py - by * px;
  c.measure = c.closed ? (u64)(px * px + py * py) : (u64)(cross < 0 ? -cross : cross);
  c.d2 = (u64)(bx * bx + by * by);
  c.index = lattice_index(p, W);
  return c;
}

__device__ __forceinline__ bool round_is_idle(const int32_t* before) { return before && *before == 0; }

// The candidates of a wave mostly share a segment: the lanes on the first active lane's slot reduce among themselves and send
// one atomic, the others their own.  `op_max`: maximum, else minimum.
template <bool op_max>
__device__ __forceinline__ void wave_atomic(u64* slots, int lo, u64 v) {
  const u64 active = __ballot(lo >= 0);
  if (!active) return;
  const int lead = __ffsll((long long)active) - 1;
  const int lo0 = __shfl(lo, lead, 64);
  u64 shared = lo == lo0 ? v : op_max ? 0ull : ~0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 other = __shfl_xor(shared, o, 64);
    shared = op_max ? (other > shared ? other : shared) : (other < shared ? other : shared);
  }
  const bool own = lo >= 0 && lo != lo0;
  if ((int)(threadIdx.x & 63) == lead || own) {
    if (op_max) __hip_atomic_fetch_max(slots + (own ? lo : lo0), own ? v : shared, RLX_AGENT);
    else __hip_atomic_fetch_min(slots + (own ? lo : lo0), own ? v : shared, RLX_AGENT);
  }
}

__global__ __launch_bounds__(256) void simplify_argmax_kernel(const int2* __restrict__ dense, int W, int D, int32_t* seg, u64* key,
                                                              const int32_t* before) {
  if (round_is_idle(before)) return;
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < D) seg[2 * (int64_t)D + k] = -1;      // the winner of the segment that starts here: none yet
  const Candidate c = candidate(dense, seg, D, W, k);
  wave_atomic<true>(key, c.lo, c.closed ? c.measure : c.packed());
}

// a == b: the measure alone stands in key; the smallest lattice index among the candidates that reach it goes to the min slot
__global__ __launch_bounds__(256) void simplify_closed_min_kernel(const int2* __restrict__ dense, int W, int D, int32_t* seg,
                                                                  const u64* __restrict__ key) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const Candidate c = candidate(dense, seg, D, W, k);
  if (c.lo >= 0 && c.closed && c.measure == key[c.lo])
    __hip_atomic_fetch_min((uint32_t*)seg + 3 * (int64_t)D + c.lo, c.index, RLX_AGENT);
}

// c^2 * 2^16 > tol_q8^2 * |b - a|^2, or |p - a|^2 * 2^16 > tol_q8^2, in 128 bits
__device__ __forceinline__ bool passes(const Candidate& c, u64 tol2) {
  const u64 left = c.closed ? c.measure : c.measure * c.measure;      // < 2^58
  const u64 left_hi = left >> 48, left_lo = left << 16;
  const u64 right_hi = c.closed ? 0ull : __umul64hi(tol2, c.d2), right_lo = c.closed ? tol2 : tol2 * c.d2;
  return left_hi > right_hi || (left_hi == right_hi && left_lo > right_lo);
}

__global__ __launch_bounds__(256) void simplify_test_kernel(const int2* __restrict__ dense, int W, int D, u64 tol2, uint8_t* __restrict__ kept,
                                                            int32_t* seg, const u64* __restrict__ key, const int32_t* before,
                                                            int32_t* raised) {
  if (round_is_idle(before)) return;
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const Candidate c = candidate(dense, seg, D, W, k);
  bool keep = false;
  if (c.lo >= 0) {
    const bool winner = c.closed ? c.measure == key[c.lo] && c.index == (uint32_t)seg[3 * (int64_t)D + c.lo] : c.packed() == key[c.lo];
    keep = winner && passes(c, tol2);
    if (keep) {
      kept[k] = 1;
      seg[2 * (int64_t)D + c.lo] = (int)k;
    }
  }
  if (__ballot(keep) && (threadIdx.x & 63) == 0) *raised = 1;      // every writer stores the same 1
}

__global__ __launch_bounds__(256) void simplify_split_kernel(int D, int32_t* seg, u64* __restrict__ key, const int32_t* before) {
  if (round_is_idle(before)) return;
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= D) return;
  key[k] = 0;
  seg[3 * (int64_t)D + k] = -1;
  const int lo = seg[k];
  if (!in_range(lo, D)) return;
  const int w = seg[2 * (int64_t)D + lo];
  if (!in_range(w, D) || w == k) {      // the segment kept nothing, or this is the kept vertex: no candidate any more
    seg[k] = -1;
    return;
  }
  const int64_t wrap = (int64_t)1 << 32;
  const int64_t ord_k = k < lo ? k + wrap : k, ord_w = w < lo ? w + wrap : (int64_t)w;
  if (ord_k < ord_w) seg[(int64_t)D + k] = w;
  else seg[k] = w;
}

// ------------------------------------------------------------------ 5. write
__global__ __launch_bounds__(256) void simplify_flags_kernel(int D, const uint8_t* __restrict__ kept, uint32_t* __restrict__ scan) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;      // the grid covers D + 1
  if (k <= D) scan[k] = k < D && kept[k] != 0;
}

__global__ __launch_bounds__(256) void simplify_scatter_kernel(const int2* __restrict__ dense, const int32_t* __restrict__ dense_offsets, int R,
                                                               int D, const uint8_t* __restrict__ kept, const uint32_t* __restrict__ scan,
                                                               int2* __restrict__ out_vertices, int32_t* __restrict__ out_offsets) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;      // the grid covers max(D, R + 1)
  if (k < D && kept[k] && in_range((int)scan[k], D)) out_vertices[scan[k]] = dense[k];
  if (k <= R) {
    const int d = dense_offsets[k];
    out_offsets[k] = (int)scan[(unsigned)d <= (unsigned)D ? d : D];
  }
}

int check_rings(const char* fn, int H, int W, int R, int V) {
  if (const int bad = check_raster(fn, H, W, RING_RASTER)) return bad;
  GDL_CHECK_ARG(R >= 0 && V >= 0 && V <= 4 * (int64_t)H * W && 4 * (int64_t)R <= V && (R == 0) == (V == 0),
                "%s: %d rings and %d vertices do not belong together", fn, R, V);
  return GDL_OK;
}

}  // namespace

extern "C" int gdl_scene_nodes(const uint8_t* mask, int H, int W, int ignore_label, const uint8_t* keep, uint8_t* nodes,
                               gdl_stream_t stream) {
  GDL_CHECK_ARG(mask && keep && nodes, "gdl_scene_nodes: null pointer");
  if (const int bad = check_raster("gdl_scene_nodes", H, W, RING_RASTER)) return bad;
  if (const int bad = check_ignore_label("gdl_scene_nodes", ignore_label)) return bad;
  hipLaunchKernelGGL(simplify_nodes_kernel, dim3(grid_for((int64_t)(H + 1) * (W + 1))), dim3(256), 0, (hipStream_t)stream,
                     Raster{mask, keep, H, W, ignore_label}, nodes);
  GDL_CHECK_LAUNCH("gdl_scene_nodes");
  return GDL_OK;
}

extern "C" int gdl_scene_simplify_count(const uint8_t* nodes, int H, int W, const int32_t* vertices, const int32_t* ring_offsets,
                                        int n_rings, int n_vertices, int32_t* pos, int32_t* bsum, int32_t* n_dense, gdl_stream_t stream) {
  GDL_CHECK_ARG(n_dense, "gdl_scene_simplify_count: null pointer");
  if (const int bad = check_rings("gdl_scene_simplify_count", H, W, n_rings, n_vertices)) return bad;
  hipStream_t s = (hipStream_t)stream;
  if (n_rings == 0) {
    if (hipMemsetAsync(n_dense, 0, sizeof(int32_t), s) != hipSuccess) GDL_CHECK_LAUNCH("gdl_scene_simplify_count");
    return GDL_OK;
  }
  GDL_CHECK_ARG(nodes && vertices && ring_offsets && pos && bsum, "gdl_scene_simplify_count: null pointer");
  const int64_t L = (int64_t)n_vertices + 1;
  hipLaunchKernelGGL(simplify_count_kernel, one_per_thread(L), dim3(256), 0, s, nodes, H, W, (const int2*)vertices, ring_offsets, n_rings,
                     n_vertices, (uint32_t*)pos);
  scan_exclusive((uint32_t*)pos, 1, L, (uint32_t*)bsum, (uint32_t*)n_dense, s);
  GDL_CHECK_LAUNCH("gdl_scene_simplify_count");
  return GDL_OK;
}

extern "C" int gdl_scene_simplify_dense(const uint8_t* nodes, int H, int W, const int32_t* vertices, const int32_t* ring_offsets,
                                        int n_rings, int n_vertices, const int32_t* pos, int n_dense, int32_t* dense,
                                        int32_t* dense_offsets, uint8_t* kept, int32_t* seg, int64_t* key, int32_t* work,
                                        gdl_stream_t stream) {
  GDL_CHECK_ARG(nodes && vertices && ring_offsets && pos && dense && dense_offsets && kept && seg && key && work,
                "gdl_scene_simplify_dense: null pointer");
  if (const int bad = check_rings("gdl_scene_simplify_dense", H, W, n_rings, n_vertices)) return bad;
  GDL_CHECK_ARG(n_rings > 0, "gdl_scene_simplify_dense: no rings");
  GDL_CHECK_ARG(n_dense >= n_vertices && n_dense <= 4 * (int64_t)H * W, "gdl_scene_simplify_dense: %d dense vertices of %d vertices", n_dense,
                n_vertices);
  hipStream_t s = (hipStream_t)stream;
  const int R = n_rings, V = n_vertices, D = n_dense;
  u64* ring_min = (u64*)work;
  uint32_t* A = (uint32_t*)work + 2 * (int64_t)R;
  int32_t* alist = work + 2 * (int64_t)R + D + 1;
  uint32_t* bsum = (uint32_t*)alist + D;
  const dim3 per_dense = one_per_thread(D);
  if (hipMemsetAsync(ring_min, 0xff, (size_t)R * sizeof(u64), s) != hipSuccess) GDL_CHECK_LAUNCH("gdl_scene_simplify_dense");
  hipLaunchKernelGGL(simplify_dense_kernel, one_per_thread(V), dim3(256), 0, s, nodes, H, W, (const int2*)vertices, ring_offsets, R, V, pos, D,
                     (int2*)dense, kept, A);
  hipLaunchKernelGGL(simplify_offsets_kernel, one_per_thread((int64_t)R + 1), dim3(256), 0, s, ring_offsets, R, V, pos, D, dense_offsets);
  scan_exclusive(A, 1, (int64_t)D + 1, bsum, nullptr, s);
  hipLaunchKernelGGL(simplify_anchor_list_kernel, per_dense, dim3(256), 0, s, D, (const uint8_t*)kept, (const uint32_t*)A, alist);
  hipLaunchKernelGGL(simplify_free_min_kernel, per_dense, dim3(256), 0, s, (const int2*)dense, (const int32_t*)dense_offsets, R, D, W,
                     (const uint32_t*)A, ring_min);
  hipLaunchKernelGGL(simplify_arcs_kernel, per_dense, dim3(256), 0, s, (const int32_t*)dense_offsets, R, D, (const uint32_t*)A,
                     (const int32_t*)alist, (const u64*)ring_min, kept, seg, (u64*)key);
  GDL_CHECK_LAUNCH("gdl_scene_simplify_dense");
  return GDL_OK;
}

extern "C" int gdl_scene_simplify_rounds(const int32_t* dense, int W, int n_dense, int tol_q8, int first, int n_rounds, uint8_t* kept,
                                         int32_t* seg, int64_t* key, int32_t* changed, gdl_stream_t stream) {
  GDL_CHECK_ARG(dense && kept && seg && key && changed, "gdl_scene_simplify_rounds: null pointer");
  GDL_CHECK_ARG(W > 0 && W < (1 << 29) && n_dense > 0, "gdl_scene_simplify_rounds: bad sizes");
  GDL_CHECK_ARG(tol_q8 >= 0 && tol_q8 <= (1 << 28), "gdl_scene_simplify_rounds: tol_q8 %d is not in 0..2^28", tol_q8);
  GDL_CHECK_ARG(n_rounds >= 1 && n_rounds <= GDL_SCENE_SIMPLIFY_ROUNDS, "gdl_scene_simplify_rounds: n_rounds %d is not in 1..%d", n_rounds,
                GDL_SCENE_SIMPLIFY_ROUNDS);
  hipStream_t s = (hipStream_t)stream;
  const int D = n_dense;
  int32_t* flags = seg + 4 * (int64_t)D;
  const dim3 grid = one_per_thread(D);
  const u64 tol2 = (u64)tol_q8 * (u64)tol_q8;
  if (hipMemsetAsync(flags, 0, GDL_SCENE_SIMPLIFY_ROUNDS * sizeof(int32_t), s) != hipSuccess ||
      hipMemsetAsync(changed, 0, sizeof(int32_t), s) != hipSuccess)
    GDL_CHECK_LAUNCH("gdl_scene_simplify_rounds");
  for (int r = 0; r < n_rounds; ++r) {
    const int32_t* before = r > 0 ? flags + (r - 1) : nullptr;      // a round after one that kept nothing returns at once
    int32_t* raised = r == n_rounds - 1 ? changed : flags + r;
    hipLaunchKernelGGL(simplify_argmax_kernel, grid, dim3(256), 0, s, (const int2*)dense, W, D, seg, (u64*)key, before);
    if (first && r == 0)      // a closed arc splits into two open ones or dies: none is left after the first round of all
      hipLaunchKernelGGL(simplify_closed_min_kernel, grid, dim3(256), 0, s, (const int2*)dense, W, D, seg, (const u64*)key);
    hipLaunchKernelGGL(simplify_test_kernel, grid, dim3(256), 0, s, (const int2*)dense, W, D, tol2, kept, seg, (const u64*)key, before, raised);
    hipLaunchKernelGGL(simplify_split_kernel, grid, dim3(256), 0, s, D, seg, (u64*)key, before);
  }
  GDL_CHECK_LAUNCH("gdl_scene_simplify_rounds");
  return GDL_OK;
}

extern "C" int gdl_scene_simplify_write(const int32_t* dense, const int32_t* dense_offsets, int n_rings, int n_dense, const uint8_t* kept,
                                        int32_t* scan, int32_t* out_vertices, int32_t* out_offsets, int32_t* n_out, gdl_stream_t stream) {
  GDL_CHECK_ARG(out_offsets && n_out, "gdl_scene_simplify_write: null pointer");
  GDL_CHECK_ARG(n_rings >= 0 && n_dense >= 0 && 4 * (int64_t)n_rings <= n_dense, "gdl_scene_simplify_write: %d rings and %d dense vertices do not belong together",
                n_rings, n_dense);
  hipStream_t s = (hipStream_t)stream;
  if (n_rings == 0 || n_dense == 0) {
    if (hipMemsetAsync(out_offsets, 0, ((size_t)n_rings + 1) * sizeof(int32_t), s) != hipSuccess ||
        hipMemsetAsync(n_out, 0, sizeof(int32_t), s) != hipSuccess)
      GDL_CHECK_LAUNCH("gdl_scene_simplify_write");
    return GDL_OK;
  }
  GDL_CHECK_ARG(dense && dense_offsets && kept && scan && out_vertices, "gdl_scene_simplify_write: null pointer");
  const int R = n_rings, D = n_dense;
  const int64_t L = (int64_t)D + 1;
  hipLaunchKernelGGL(simplify_flags_kernel, one_per_thread(L), dim3(256), 0, s, D, kept, (uint32_t*)scan);
  scan_exclusive((uint32_t*)scan, 1, L, (uint32_t*)scan + L, (uint32_t*)n_out, s);
  hipLaunchKernelGGL(simplify_scatter_kernel, one_per_thread(D > R + 1 ? D : R + 1), dim3(256), 0, s, (const int2*)dense, dense_offsets, R, D,
                     kept, (const uint32_t*)scan, (int2*)out_vertices, out_offsets);
  GDL_CHECK_LAUNCH("gdl_scene_simplify_write");
  return GDL_OK;
}
