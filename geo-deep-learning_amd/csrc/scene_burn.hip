// Polygon rings burned into a label raster (include/gdlhip_scene_burn.h): the crossings of the rings' edges with the centre
// lines of the raster rows, added to two difference planes and summed along each row.
//
//   gdl_scene_burn_count: a thread per offset counts the bad ones; a thread per vertex finds the ring of the edge that leaves it
//     (binary search in ring_offsets), counts its bad coordinates and writes the number of raster rows the edge crosses; their
//     exclusive scan (scan_u32.h) is edge_rows, and their 64-bit sum, reduced in the wave, goes to counts[0].
//   gdl_scene_burn_fill: three kinds of launch.
//       a. the plane (C, S) and the two counts are zeroed;
//       b. a thread per crossing k: the edge is the last e with edge_rows[e] <= k, the row is the edge's first row plus
//          k - edge_rows[e], the column follows from the header's integer quotient; two int32 atomics, C += w and S += w * value;
//       c. a workgroup per row: a thread per pixel of a chunk of CHUNK, the inclusive scans of C and S inside the wave by
//          shuffles, the waves' totals through LDS (double buffered: one barrier per chunk) and the carry of the chunks before in
//          a register; the pixel is resolved, stored and counted, and a wave adds its counts with one atomic each at the end.
//
// No thread walks an edge: a traced ring's vertical run can span the whole scene.  No workgroup waits for another anywhere;
// every loop has a trip count its comment states.  Every sum is an integer add, so no result depends on any order.  The
// crossing kernel checks the ring, the edge and the row it derives against the vertices themselves and drops what does not
// fit, so arrays that do not belong together give wrong numbers but touch nothing outside the plane.
#include <climits>

#include "gdl_common.h"
#include "../../include/gdlhip_scene_burn.h"

namespace {

#include "scan_u32.h"
#include "scene_common.h"
static_assert(SCAN_TILE == GDL_SCENE_BURN_SCAN_TILE, "the header states the scan's block size for the callers' scratch");

constexpr int CHUNK = GDL_SCENE_BURN_CHUNK;      // the pixels of a row per turn: one per thread of the workgroup
constexpr int COORD_BITS = 20;                   // |c| <= 2^COORD_BITS pixels
static_assert(CHUNK == 256 && GDL_SCENE_BURN_BITS_MAX == 8, "a thread is a pixel; 2^62 bounds the quotient's terms");

__device__ __forceinline__ int64_t ceil_div(int64_t a, int64_t b) {      // b > 0
  const int64_t q = a / b;
  return q + (a % b > 0);
}

__device__ __forceinline__ bool coord_ok(int c, int bits) {
  const int lim = 1 << (COORD_BITS + bits);
  return c >= -lim && c <= lim;
}

// An edge in doubled units, or none: `ok` is false for a vertex outside every ring, a ring of fewer than 3 vertices, offsets
// that do not bracket the vertex inside 0 .. V, a bad coordinate and a flat edge.
struct Edge {
  bool ok; int ring; int64_t ax, ay, bx, by;
};

// the edge that leaves vertex e, r its ring as far as known (any int: it is checked)
__device__ __forceinline__ Edge load_edge(const int32_t* __restrict__ vertices, const int32_t* __restrict__ ring_offsets, int R, int V,
                                          int bits, int e, int r) {
  Edge g{false, r, 0, 0, 0, 0};
  if ((unsigned)r >= (unsigned)R || (unsigned)e >= (unsigned)V) return g;
  const int o0 = ring_offsets[r], o1 = ring_offsets[r + 1];
  if (o0 < 0 || o1 > V || e < o0 || e >= o1 || o1 - o0 < 3) return g;
  const int n = e + 1 == o1 ? o0 : e + 1;
  const int ax = vertices[2 * (int64_t)e], ay = vertices[2 * (int64_t)e + 1], bx = vertices[2 * (int64_t)n], by = vertices[2 * (int64_t)n + 1];
  if (!coord_ok(ax, bits) || !coord_ok(ay, bits) || !coord_ok(bx, bits) || !coord_ok(by, bits) || ay == by) return g;
  g.ok = true; g.ax = 2 * (int64_t)ax; g.ay = 2 * (int64_t)ay; g.bx = 2 * (int64_t)bx; g.by = 2 * (int64_t)by;
  return g;
}

// the raster rows y0 .. y1 - 1 the edge crosses: min(ay, by) <= (2 y + 1) u < max(ay, by), clipped to 0 .. H
__device__ __forceinline__ void edge_span(const Edge& g, int bits, int H, int64_t& y0, int64_t& y1) {
  const int64_t lo = g.ay < g.by ? g.ay : g.by, hi = g.ay < g.by ? g.by : g.ay, u = (int64_t)1 << bits;
  y0 = (lo - u + 2 * u - 1) >> (bits + 1);      // ceil((lo - u) / 2u): the first y with (2 y + 1) u >= lo
  y1 = (hi - u + 2 * u - 1) >> (bits + 1);      // the first y with (2 y + 1) u >= hi
  y0 = y0 < 0 ? 0 : (y0 > H ? H : y0);
  y1 = y1 < 0 ? 0 : (y1 > H ? H : y1);
}

// ------------------------------------------------------------------ count
__global__ __launch_bounds__(256) void burn_offsets_kernel(const int32_t* __restrict__ ring_offsets, int R, int V, int64_t* __restrict__ counts) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r <= R; r += (int64_t)gridDim.x * 256) {      // ceil((R + 1) / threads) turns
    const int o = ring_offsets[r];
    if (o < 0 || o > V || (r > 0 && o < ring_offsets[r - 1])) __hip_atomic_fetch_add(counts + 1, (int64_t)1, RLX_AGENT);
  }
}

__global__ __launch_bounds__(256) void burn_edges_kernel(const int32_t* __restrict__ vertices, const int32_t* __restrict__ ring_offsets, int R,
                                                         int V, int bits, int H, int32_t* __restrict__ edge_ring,
                                                         uint32_t* __restrict__ edge_rows, int64_t* __restrict__ counts) {
  int64_t rows = 0, bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= V; i += (int64_t)gridDim.x * 256) {      // ceil((V + 1) / threads) turns
    if (i == V) { edge_rows[i] = 0; break; }
    const int e = (int)i;
    bad += !coord_ok(vertices[2 * i], bits) + !coord_ok(vertices[2 * i + 1], bits);
    // the last ring r with ring_offsets[r] <= e; -1 where the first offset lies above e
    int lo = -1, hi = R;
    while (hi - lo > 1) {      // at most 31 turns
      const int mid = lo + (hi - lo) / 2;
      if (ring_offsets[mid] <= e) lo = mid; else hi = mid;
    }
    const Edge g = load_edge(vertices, ring_offsets, R, V, bits, e, lo);
    int64_t y0 = 0, y1 = 0;
    if (g.ok) edge_span(g, bits, H, y0, y1);
    edge_ring[e] = g.ok || ((unsigned)lo < (unsigned)R && e < ring_offsets[lo + 1]) ? lo : -1;
    edge_rows[e] = (uint32_t)(y1 - y0);
    rows += y1 - y0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {      // 6 turns
    rows += __shfl_xor(rows, o, 64);
    bad += __shfl_xor(bad, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (rows) __hip_atomic_fetch_add(counts, rows, RLX_AGENT);
    if (bad) __hip_atomic_fetch_add(counts + 1, bad, RLX_AGENT);
  }
}

// ------------------------------------------------------------------ fill
// n int32 of plane (16-byte aligned) and the two counts
__global__ __launch_bounds__(256) void burn_zero_kernel(int32_t* __restrict__ plane, int64_t n, int64_t* __restrict__ counts) {
  if (blockIdx.x == 0 && threadIdx.x < 2) counts[threadIdx.x] = 0;
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)      // ceil(n4 / threads) turns
    ((int4*)plane)[i] = make_int4(0, 0, 0, 0);
  if (blockIdx.x == 0 && threadIdx.x < n - 4 * n4) plane[4 * n4 + threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void burn_cross_kernel(const int32_t* __restrict__ vertices, const int32_t* __restrict__ ring_offsets,
                                                         const uint8_t* __restrict__ value, int R, int V, int bits, int H, int W,
                                                         const int32_t* __restrict__ edge_ring, const uint32_t* __restrict__ edge_rows,
                                                         int64_t n_cross, int32_t* __restrict__ plane) {
  const int64_t HW = (int64_t)H * W;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n_cross; k += (int64_t)gridDim.x * 256) {      // ceil(n_cross / threads) turns
    // the last edge e in 0 .. V - 1 with edge_rows[e] <= k (edge_rows[0] == 0)
    int lo = 0, hi = V;
    while (hi - lo > 1) {      // at most 31 turns
      const int mid = lo + (hi - lo) / 2;
      if (edge_rows[mid] <= (uint32_t)k) lo = mid; else hi = mid;
    }
    const Edge g = load_edge(vertices, ring_offsets, R, V, bits, lo, edge_ring[lo]);
    if (!g.ok) continue;
    int64_t y0, y1;
    edge_span(g, bits, H, y0, y1);
    const int64_t y = y0 + (k - (int64_t)edge_rows[lo]);
    if (y < y0 || y >= y1) continue;
    const int64_t u = (int64_t)1 << bits, cy = (2 * y + 1) * u, dy = g.by - g.ay, dx = g.bx - g.ax;
    const int64_t ady = dy < 0 ? -dy : dy, P = (dy < 0 ? -1 : 1) * (g.ax * dy + (cy - g.ay) * dx);
    int64_t x0 = ceil_div(P - ady * u, 2 * ady * u);
    if (x0 >= W) continue;
    x0 = x0 < 0 ? 0 : x0;
    const int w = dy < 0 ? 1 : -1;
    __hip_atomic_fetch_add(plane + y * W + x0, w, RLX_AGENT);
    __hip_atomic_fetch_add(plane + HW + y * W + x0, w * (int)value[g.ring], RLX_AGENT);
  }
}

// what a pixel becomes, and whether it counts as a conflict
__device__ __forceinline__ int resolve(int c, int s, int background, int conflict, int& conflicts) {
  if (c == 1 && s >= 0 && s <= 255) return s;
  if (c == 0 && s == 0) return background;
  ++conflicts;
  return conflict;
}

// one workgroup per row (blockIdx.x; rows beyond the grid by stride)
__global__ __launch_bounds__(256) void burn_rows_kernel(const int32_t* __restrict__ plane, int H, int W, int background, int conflict,
                                                        const uint8_t* __restrict__ reference, uint8_t* __restrict__ out,
                                                        int64_t* __restrict__ counts) {
  __shared__ int wc[2][4], ws[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t HW = (int64_t)H * W;
  int conflicts = 0, differ = 0, turn = 0;
  for (int y = blockIdx.x; y < H; y += gridDim.x) {      // ceil(H / workgroups) turns
    const int64_t row = (int64_t)y * W;
    int carry_c = 0, carry_s = 0;
    for (int x0 = 0; x0 < W; x0 += CHUNK, turn ^= 1) {      // ceil(W / CHUNK) turns
      const int x = x0 + threadIdx.x;
      int c = x < W ? plane[row + x] : 0, s = x < W ? plane[HW + row + x] : 0;
      const int ref = reference && x < W ? reference[row + x] : 0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {      // 6 turns
        const int uc = __shfl_up(c, o, 64), us = __shfl_up(s, o, 64);
        if (lane >= o) { c += uc; s += us; }
      }
      if (lane == 63) { wc[turn][wave] = c; ws[turn][wave] = s; }
      __syncthreads();      // the one barrier of the turn: the next turn writes the other buffer
      int tot_c = 0, tot_s = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {      // 4 turns
        const int vc = wc[turn][w], vs = ws[turn][w];
        tot_c += vc; tot_s += vs;
        if (w < wave) { c += vc; s += vs; }
      }
      c += carry_c; s += carry_s;
      carry_c += tot_c; carry_s += tot_s;
      if (x < W) {
        const int v = resolve(c, s, background, conflict, conflicts);
        out[row + x] = (uint8_t)v;
        differ += reference && v != ref;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {      // 6 turns
    conflicts += __shfl_xor(conflicts, o, 64);
    differ += __shfl_xor(differ, o, 64);
  }
  if (lane == 0) {
    if (conflicts) __hip_atomic_fetch_add(counts, (int64_t)conflicts, RLX_AGENT);
    if (differ) __hip_atomic_fetch_add(counts + 1, (int64_t)differ, RLX_AGENT);
  }
}

// no crossing: the background everywhere, and how far that is from the reference
__global__ __launch_bounds__(256) void burn_background_kernel(int64_t HW, int background, const uint8_t* __restrict__ reference,
                                                              uint8_t* __restrict__ out, int64_t* __restrict__ counts) {
  int64_t differ = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {      // ceil(HW / threads) turns
    out[i] = (uint8_t)background;
    differ += reference && reference[i] != background;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) differ += __shfl_xor(differ, o, 64);      // 6 turns
  if ((threadIdx.x & 63) == 0 && differ) __hip_atomic_fetch_add(counts + 1, differ, RLX_AGENT);
}

int check_common(const char* fn, int n_rings, int n_vertices, int bits, int H, int W) {
  if (const int bad = check_raster(fn, H, W, LINEAR_INDEX)) return bad;
  GDL_CHECK_ARG(bits >= 0 && bits <= GDL_SCENE_BURN_BITS_MAX, "%s: bits must be in 0..%d, got %d", fn, GDL_SCENE_BURN_BITS_MAX, bits);
  GDL_CHECK_ARG(n_rings >= 0 && n_vertices >= 0 && n_vertices < INT32_MAX, "%s: %d rings and %d vertices", fn, n_rings, n_vertices);
  return GDL_OK;
}

}  // namespace

extern "C" int gdl_scene_burn_count(const int32_t* vertices, const int32_t* ring_offsets, int n_rings, int n_vertices, int bits, int H,
                                    int W, int32_t* edge_ring, int32_t* edge_rows, int32_t* bsum, int64_t* counts, gdl_stream_t stream) {
  if (const int bad = check_common("gdl_scene_burn_count", n_rings, n_vertices, bits, H, W)) return bad;
  GDL_CHECK_ARG(ring_offsets && edge_rows && bsum && counts && (n_vertices == 0 || (vertices && edge_ring)),
                "gdl_scene_burn_count: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int R = n_rings, V = n_vertices;
  if (hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s) != hipSuccess) GDL_CHECK_LAUNCH("gdl_scene_burn_count");
  hipLaunchKernelGGL(burn_offsets_kernel, dim3(grid_for((int64_t)R + 1)), dim3(256), 0, s, ring_offsets, R, V, counts);
  hipLaunchKernelGGL(burn_edges_kernel, dim3(grid_for((int64_t)V + 1)), dim3(256), 0, s, vertices, ring_offsets, R, V, bits, H, edge_ring,
                     (uint32_t*)edge_rows, counts);
  scan_exclusive((uint32_t*)edge_rows, 1, (int64_t)V + 1, (uint32_t*)bsum, nullptr, s);
  GDL_CHECK_LAUNCH("gdl_scene_burn_count");
  return GDL_OK;
}

extern "C" int gdl_scene_burn_fill(const int32_t* vertices, const int32_t* ring_offsets, const uint8_t* value, int n_rings, int n_vertices,
                                   int bits, int H, int W, const int32_t* edge_ring, const int32_t* edge_rows, int64_t n_cross,
                                   int background, int conflict, const uint8_t* reference, int32_t* plane, uint8_t* out, int64_t* counts,
                                   gdl_stream_t stream) {
  if (const int bad = check_common("gdl_scene_burn_fill", n_rings, n_vertices, bits, H, W)) return bad;
  GDL_CHECK_ARG(background >= 0 && background <= 255 && conflict >= 0 && conflict <= 255,
                "gdl_scene_burn_fill: background and conflict must be in 0..255, got %d and %d", background, conflict);
  GDL_CHECK_ARG(n_cross >= 0 && n_cross <= INT32_MAX, "gdl_scene_burn_fill: %lld crossings: their scan is 32 bits wide (n_cross < 2^31)",
                (long long)n_cross);
  GDL_CHECK_ARG(out && counts, "gdl_scene_burn_fill: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  if (n_cross == 0 || n_rings == 0 || n_vertices == 0) {
    hipLaunchKernelGGL(burn_zero_kernel, dim3(1), dim3(256), 0, s, (int32_t*)nullptr, (int64_t)0, counts);
    hipLaunchKernelGGL(burn_background_kernel, dim3(grid_for(HW)), dim3(256), 0, s, HW, background, reference, out, counts);
    GDL_CHECK_LAUNCH("gdl_scene_burn_fill");
    return GDL_OK;
  }
  GDL_CHECK_ARG(vertices && ring_offsets && value && edge_ring && edge_rows && plane, "gdl_scene_burn_fill: null pointer");
  GDL_CHECK_ARG((uintptr_t)plane % 16 == 0, "gdl_scene_burn_fill: plane must be 16-byte aligned");
  hipLaunchKernelGGL(burn_zero_kernel, dim3(grid_for(HW / 2)), dim3(256), 0, s, plane, 2 * HW, counts);
  hipLaunchKernelGGL(burn_cross_kernel, dim3(grid_for(n_cross)), dim3(256), 0, s, vertices, ring_offsets, value, n_rings, n_vertices, bits,
                     H, W, edge_ring, (const uint32_t*)edge_rows, n_cross, plane);
  hipLaunchKernelGGL(burn_rows_kernel, dim3((unsigned)(H < 65536 ? H : 65536)), dim3(256), 0, s, (const int32_t*)plane, H, W, background,
                     conflict, reference, out, counts);
  GDL_CHECK_LAUNCH("gdl_scene_burn_fill");
  return GDL_OK;
}
