// Polygon rings of a label mask (include/gdlhip_scene_rings.h): the cycles of the successor permutation over the boundary sides
// of the mask's regions, found by list ranking.  Definitions (lattice, sides, slots, successor, canonical ring) are the header's.
//
// Whether a side is a boundary side, and so the compact index of any slot, is a function of the mask around the pixel and of
// `offsets`; nothing of 4 * H * W entries exists.  The launches, each seeing the stores of the one before through the kernel
// boundary (E boundary sides, rounds = ceil(log2(E))):
//   count   rings_count (boundary sides per pixel), then the exclusive scan of scan_u32.h over H * W -> offsets, E
//   trace   rings_fill          per pixel: slot and successor of its boundary sides; m = e, j = next
//           rings_min_round     x rounds: m' = min(m, m[j]), j' = j[j] -> side_ring, the smallest compact index of the cycle
//           rings_rank_init     d = corner flag, j = next, or -1 where next is the ring's start (the cycle cut open)
//           rings_rank_round    x rounds: d' = d + d[j], j' = j[j] while j >= 0 -> side_rank
//           rings_starts        is-start and vertex count per side, then one scan of both over E -> ring index, first vertex, R, V
//   write   rings_write         per side: the ring's scalars from its start side, a vertex from a corner side, area2 by atomics
// The doublings never work in place: a round reads one buffer pair and writes the other, and the pair the last round writes is
// the output array (the parity of `rounds` picks which buffer starts).  A round raises flags[round] when it changed an entry it
// looks at (m for the minimum, anything for the rank); a round that finds the flag of the round before it down returns at once.
// That is sound because a round that changes nothing has written its input out again: both buffers then hold the final values
// (for the minimum: m' == m everywhere means m is constant along the orbits of j, whose windows cover the cycle).
// No workgroup waits for another and there is no host read inside an entry point.  The only loops are grid-stride sweeps over the
// pixels and the four sides of a pixel: every kernel ends whatever the input.
#include "gdl_common.h"
#include "../../include/gdlhip_scene_rings.h"

namespace {

#include "scan_u32.h"
#include "scene_common.h"
static_assert(SCAN_TILE == GDL_SCENE_RINGS_SCAN_TILE, "the header states the scan's block size for the callers' scratch");

// d_s, the direction of travel of side s: E, S, W, N.  The outward normal n_s is d_{(s + 3) % 4}.
__device__ __forceinline__ int dir_x(int s) { return s == 0 ? 1 : s == 2 ? -1 : 0; }
__device__ __forceinline__ int dir_y(int s) { return s == 1 ? 1 : s == 3 ? -1 : 0; }

// v is the value of a live pixel (Raster, scene_common.h): a cell holds it exactly when it is a live pixel of that value
__device__ __forceinline__ bool same(const Raster& r, int y, int x, int v) { return r.inside(y, x) && r.mask[(int64_t)y * r.W + x] == v; }
// bit s: side s of the live pixel (y, x) of value v is a boundary side
__device__ __forceinline__ int boundary(const Raster& r, int y, int x, int v) {
  return (int)!same(r, y - 1, x, v) | (int)!same(r, y, x + 1, v) << 1 | (int)!same(r, y + 1, x, v) << 2 | (int)!same(r, y, x - 1, v) << 3;
}

// ------------------------------------------------------------------ 1. count
__global__ __launch_bounds__(256) void rings_count_kernel(Raster r, uint32_t* __restrict__ offsets) {
  const int64_t HW = (int64_t)r.H * r.W;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
    const int y = (int)(p / r.W), x = (int)(p % r.W);
    const int v = r.live(y, x);
    offsets[p] = v < 0 ? 0u : (uint32_t)__popc(boundary(r, y, x, v));
  }
}

// ------------------------------------------------------------------ 2. trace
// One thread per pixel writes the entries of its boundary sides.  The successor (q, t) of a side is a boundary side of q, so its
// compact index is offsets[q] plus the boundary sides of q below t.  A compact index outside 0 .. E - 1 can only come from
// offsets that belong to another mask: such a side is not written and such a successor is bent back to the side itself, so that
// the gathers of the rounds below stay inside their arrays whatever the caller passed.
__global__ __launch_bounds__(256) void rings_fill_kernel(Raster r, int conn8, const int32_t* __restrict__ offsets, int E,
                                                         int32_t* __restrict__ side_slot, int32_t* __restrict__ side_next,
                                                         int32_t* __restrict__ m, int32_t* __restrict__ j) {
  const int64_t HW = (int64_t)r.H * r.W;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
    const int y = (int)(p / r.W), x = (int)(p % r.W);
    const int v = r.live(y, x);
    if (v < 0) continue;
    const int bits = boundary(r, y, x, v);
    int e = offsets[p];
    for (int s = 0; s < 4; ++s) {
      if (!(bits >> s & 1)) continue;
      const int n = (s + 3) & 3;
      const int ay = y + dir_y(s), ax = x + dir_x(s), by = ay + dir_y(n), bx = ax + dir_x(n);
      const bool same_a = same(r, ay, ax, v), same_b = same(r, by, bx, v);
      int qy = y, qx = x, t = (s + 1) & 3;      // turn on the pixel itself
      if (conn8 ? same_b : same_a && same_b) { qy = by; qx = bx; t = n; }
      else if (same_a) { qy = ay; qx = ax; t = s; }
      const int q_bits = qy == y && qx == x ? bits : boundary(r, qy, qx, v);
      int next = offsets[(int64_t)qy * r.W + qx] + __popc(q_bits & ((1 << t) - 1));
      if (e >= 0 && e < E) {
        if (next < 0 || next >= E) next = e;
        side_slot[e] = (int)(4 * p + s);
        side_next[e] = next;
        m[e] = e;
        j[e] = next;
      }
      ++e;
    }
  }
}

// the round's early exit and its flag: flags[round] goes up when a lane of the wave changed something
__device__ __forceinline__ bool round_is_idle(const int32_t* flags, int round) { return round > 0 && flags[round - 1] == 0; }
__device__ __forceinline__ void raise_flag(int32_t* flags, int round, bool changed) {
  if (__ballot(changed) && (threadIdx.x & 63) == 0) flags[round] = 1;      // every writer stores the same 1
}

__global__ __launch_bounds__(256) void rings_min_round_kernel(int E, const int32_t* __restrict__ m_in, const int32_t* __restrict__ j_in,
                                                              int32_t* __restrict__ m_out, int32_t* __restrict__ j_out, int32_t* flags,
                                                              int round) {
  if (round_is_idle(flags, round)) return;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;      // the grid covers E exactly: one side per thread
  bool changed = false;
  if (e < E) {
    const int j = in_range(j_in[e], E) ? j_in[e] : (int)e, m = m_in[e], other = m_in[j];
    changed = other < m;
    m_out[e] = changed ? other : m;
    j_out[e] = j_in[j];
  }
  raise_flag(flags, round, changed);
}

// d = 1 on a corner side (the successor has another side number), j = the successor unless that is the ring's start side
__global__ __launch_bounds__(256) void rings_rank_init_kernel(int E, const int32_t* __restrict__ side_slot, const int32_t* __restrict__ side_next,
                                                              const int32_t* __restrict__ side_ring, int32_t* __restrict__ d,
                                                              int32_t* __restrict__ j) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int next = in_range(side_next[e], E) ? side_next[e] : (int)e;
  d[e] = ((side_slot[e] ^ side_slot[next]) & 3) != 0;
  j[e] = side_ring[e] == next ? -1 : next;
}

__global__ __launch_bounds__(256) void rings_rank_round_kernel(int E, const int32_t* __restrict__ d_in, const int32_t* __restrict__ j_in,
                                                               int32_t* __restrict__ d_out, int32_t* __restrict__ j_out, int32_t* flags,
                                                               int round) {
  if (round_is_idle(flags, round)) return;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool changed = false;
  if (e < E) {
    const int j = j_in[e] < E ? j_in[e] : -1;
    changed = j >= 0;
    d_out[e] = d_in[e] + (changed ? d_in[j] : 0);
    j_out[e] = changed ? j_in[j] : -1;
  }
  raise_flag(flags, round, changed);
}

// what the scan turns into the ring's index and its first vertex, at the ring's start side; 0 at every other side
__global__ __launch_bounds__(256) void rings_starts_kernel(int E, const int32_t* __restrict__ side_ring, const int32_t* __restrict__ side_rank,
                                                           uint32_t* __restrict__ is_start, uint32_t* __restrict__ n_vertices) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const bool start = side_ring[e] == e;
  is_start[e] = start;
  n_vertices[e] = start ? (uint32_t)side_rank[e] : 0u;
}

// ------------------------------------------------------------------ 3. write
// Side (p, s) from (x0, y0) to (x1, y1) adds x0 * y1 - x1 * y0 to its ring's area2: -y, x + 1, y + 1, -x for s = 0 .. 3 (the
// collinear lattice points between two vertices add nothing to the sum over the vertices alone).  The sides of a wave mostly
// belong to one ring, so the lanes that share the first lane's ring add once.  Indices that the counts do not cover (buffers of
// another trace) are skipped, not written.
__global__ __launch_bounds__(256) void rings_write_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ labels, int W, int E,
                                                          int R, int V, const int32_t* __restrict__ side_slot,
                                                          const int32_t* __restrict__ side_next, const int32_t* __restrict__ side_ring,
                                                          const int32_t* __restrict__ side_rank, const int32_t* __restrict__ ring_index,
                                                          const int32_t* __restrict__ first_vertex, int32_t* __restrict__ vertices,
                                                          int32_t* __restrict__ ring_offsets, uint8_t* __restrict__ value,
                                                          int32_t* __restrict__ label, int32_t* __restrict__ start, int64_t* area2) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int ring = -1;
  int64_t term = 0;
  if (e < E) {
    const int first = in_range(side_ring[e], E) ? side_ring[e] : (int)e, slot = side_slot[e];
    const int p = slot >> 2, s = slot & 3, y = p / W, x = p % W;
    const int next = in_range(side_next[e], E) ? side_next[e] : (int)e;
    const int r = ring_index[first];
    if (r >= 0 && r < R) {
      ring = r;
      term = s == 0 ? -y : s == 1 ? x + 1 : s == 2 ? y + 1 : -x;
      const int v0 = first_vertex[first];
      if (first == e) {
        ring_offsets[r] = v0;
        value[r] = mask[p];
        label[r] = labels[p];
        start[r] = slot;
      }
      if ((slot ^ side_slot[next]) & 3) {      // a corner side: its head point is a vertex
        const int64_t k = (int64_t)v0 + side_rank[first] - side_rank[e];
        if (k >= 0 && k < V) {
          vertices[2 * k] = x + (s == 0 || s == 1);
          vertices[2 * k + 1] = y + (s == 1 || s == 2);
        }
      }
    }
    if (e == 0) ring_offsets[R] = V;
  }
  const unsigned long long active = __ballot(ring >= 0);
  if (active) {
    const int lead = __ffsll((long long)active) - 1;
    const int ring0 = __shfl(ring, lead, 64);
    int64_t shared = ring == ring0 ? term : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) shared += __shfl_xor(shared, o, 64);
    if ((int)(threadIdx.x & 63) == lead) __hip_atomic_fetch_add(area2 + ring0, shared, RLX_AGENT);
    else if (ring >= 0 && ring != ring0) __hip_atomic_fetch_add(area2 + ring, term, RLX_AGENT);
  }
}

int check_mask(const char* fn, int H, int W, int ignore_label) {
  if (const int bad = check_raster(fn, H, W, RING_SLOT)) return bad;
  return check_ignore_label(fn, ignore_label);
}

inline int doubling_rounds(int E) {
  int r = 0;
  while (((int64_t)1 << r) < E) ++r;
  return r;
}

}  // namespace

extern "C" int gdl_scene_rings_count(const uint8_t* mask, int H, int W, int ignore_label, const uint8_t* keep, int32_t* offsets,
                                     int32_t* bsum, int32_t* n_sides, gdl_stream_t stream) {
  GDL_CHECK_ARG(mask && keep && offsets && bsum && n_sides, "gdl_scene_rings_count: null pointer");
  if (const int bad = check_mask("gdl_scene_rings_count", H, W, ignore_label)) return bad;
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const Raster r{mask, keep, H, W, ignore_label};
  hipLaunchKernelGGL(rings_count_kernel, dim3(grid_for(HW)), dim3(256), 0, s, r, (uint32_t*)offsets);
  scan_exclusive((uint32_t*)offsets, 1, HW, (uint32_t*)bsum, (uint32_t*)n_sides, s);
  GDL_CHECK_LAUNCH("gdl_scene_rings_count");
  return GDL_OK;
}

extern "C" int gdl_scene_rings_trace(const uint8_t* mask, int H, int W, int connectivity, int ignore_label, const uint8_t* keep,
                                     const int32_t* offsets, int n_sides, int32_t* side_slot, int32_t* side_next, int32_t* side_ring,
                                     int32_t* side_rank, int32_t* work, int32_t* counts, gdl_stream_t stream) {
  GDL_CHECK_ARG(mask && keep && offsets && counts, "gdl_scene_rings_trace: null pointer");
  if (const int bad = check_mask("gdl_scene_rings_trace", H, W, ignore_label)) return bad;
  if (const int bad = check_connectivity("gdl_scene_rings_trace", connectivity)) return bad;
  const int64_t HW = (int64_t)H * W;
  GDL_CHECK_ARG(n_sides >= 0 && n_sides <= 4 * HW, "gdl_scene_rings_trace: n_sides %d is not in 0..4 * H * W", n_sides);
  hipStream_t s = (hipStream_t)stream;
  const int E = n_sides;
  if (E == 0) {
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), s) != hipSuccess) GDL_CHECK_LAUNCH("gdl_scene_rings_trace");
    return GDL_OK;
  }
  GDL_CHECK_ARG(side_slot && side_next && side_ring && side_rank && work, "gdl_scene_rings_trace: null pointer");
  const int64_t nb = ((int64_t)E + SCAN_TILE - 1) / SCAN_TILE;
  int32_t* w0 = work;
  int32_t* w1 = work + E;
  int32_t* w2 = work + 2 * (int64_t)E;
  int32_t* bsum = work + 3 * (int64_t)E;
  int32_t* flags = bsum + 2 * nb;
  const int rounds = doubling_rounds(E);      // at most 31: 2 * rounds flags fit GDL_SCENE_RINGS_FLAGS
  static_assert(GDL_SCENE_RINGS_FLAGS >= 2 * 31, "one flag per round of both doublings");
  const dim3 sides = one_per_thread(E);
  const Raster r{mask, keep, H, W, ignore_label};
  if (hipMemsetAsync(flags, 0, GDL_SCENE_RINGS_FLAGS * sizeof(int32_t), s) != hipSuccess) GDL_CHECK_LAUNCH("gdl_scene_rings_trace");

  // the buffer that round `rounds` would read, i.e. the one the last round writes, is the output array
  int32_t* val[2];
  int32_t* jmp[2] = {w0, w1};
  val[rounds & 1] = side_ring;
  val[~rounds & 1] = w2;
  hipLaunchKernelGGL(rings_fill_kernel, dim3(grid_for(HW)), dim3(256), 0, s, r, connectivity == 8, offsets, E, side_slot, side_next, val[0],
                     jmp[0]);
  for (int k = 0; k < rounds; ++k)
    hipLaunchKernelGGL(rings_min_round_kernel, sides, dim3(256), 0, s, E, (const int32_t*)val[k & 1], (const int32_t*)jmp[k & 1],
                       val[~k & 1], jmp[~k & 1], flags, k);

  val[rounds & 1] = side_rank;
  val[~rounds & 1] = w2;
  hipLaunchKernelGGL(rings_rank_init_kernel, sides, dim3(256), 0, s, E, (const int32_t*)side_slot, (const int32_t*)side_next,
                     (const int32_t*)side_ring, val[0], jmp[0]);
  for (int k = 0; k < rounds; ++k)
    hipLaunchKernelGGL(rings_rank_round_kernel, sides, dim3(256), 0, s, E, (const int32_t*)val[k & 1], (const int32_t*)jmp[k & 1],
                       val[~k & 1], jmp[~k & 1], flags + 32, k);

  hipLaunchKernelGGL(rings_starts_kernel, sides, dim3(256), 0, s, E, (const int32_t*)side_ring, (const int32_t*)side_rank, (uint32_t*)w0,
                     (uint32_t*)w1);
  scan_exclusive((uint32_t*)w0, 2, E, (uint32_t*)bsum, (uint32_t*)counts, s);      // w0 and w1 are adjacent: two segments of E
  GDL_CHECK_LAUNCH("gdl_scene_rings_trace");
  return GDL_OK;
}

extern "C" int gdl_scene_rings_write(const uint8_t* mask, const int32_t* labels, int W, int n_sides, int n_rings, int n_vertices,
                                     const int32_t* side_slot, const int32_t* side_next, const int32_t* side_ring,
                                     const int32_t* side_rank, const int32_t* work, int32_t* vertices, int32_t* ring_offsets,
                                     uint8_t* value, int32_t* label, int32_t* start, int64_t* area2, gdl_stream_t stream) {
  GDL_CHECK_ARG(ring_offsets, "gdl_scene_rings_write: null pointer");
  GDL_CHECK_ARG(W > 0 && n_sides >= 0 && n_rings >= 0 && n_vertices >= 0, "gdl_scene_rings_write: bad sizes");
  GDL_CHECK_ARG((n_sides == 0) == (n_rings == 0) && (n_rings == 0) == (n_vertices == 0) && 4 * (int64_t)n_rings <= n_vertices &&
                    n_vertices <= n_sides,
                "gdl_scene_rings_write: %d sides, %d rings and %d vertices do not belong together", n_sides, n_rings, n_vertices);
  hipStream_t s = (hipStream_t)stream;
  if (n_sides == 0) {
    if (hipMemsetAsync(ring_offsets, 0, sizeof(int32_t), s) != hipSuccess) GDL_CHECK_LAUNCH("gdl_scene_rings_write");
    return GDL_OK;
  }
  GDL_CHECK_ARG(mask && labels && side_slot && side_next && side_ring && side_rank && work && vertices && value && label && start && area2,
                "gdl_scene_rings_write: null pointer");
  if (hipMemsetAsync(area2, 0, (size_t)n_rings * sizeof(int64_t), s) != hipSuccess) GDL_CHECK_LAUNCH("gdl_scene_rings_write");
  hipLaunchKernelGGL(rings_write_kernel, one_per_thread(n_sides), dim3(256), 0, s, mask, labels, W, n_sides, n_rings, n_vertices,
                     side_slot, side_next, side_ring, side_rank, work, work + n_sides, vertices, ring_offsets, value, label, start, area2);
  GDL_CHECK_LAUNCH("gdl_scene_rings_write");
  return GDL_OK;
}
