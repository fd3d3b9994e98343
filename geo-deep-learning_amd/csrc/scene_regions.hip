// Per-region attributes of a label mask (include/gdlhip_scene_regions.h): a segmented reduction over the pixels, keyed by the
// component label of gdl_scene_components (scene_sieve.hip).
//
//   gdl_scene_regions_count: a flag per pixel (is it a root, labels[i] == i) and its exclusive scan (scan_u32.h): rank[i] is the
//     dense number of the region whose label is i, and the total is N.
//   gdl_scene_regions_stats: a fill launch (sums 0, minima INT32_MAX, maxima INT32_MIN), then one workgroup per TILE x TILE
//     pixels, thread (wave w, lane x) owning column x of rows w * 16 .. w * 16 + 15 as in scene_sieve.hip:
//       a. row runs: a ballot marks where a run of equal label starts; a run's pixel count, its x-extent and its sum of x follow
//          from its two ends, its sum and minimum of q from a segmented scan inside the wave (six shuffle steps each).  Only the
//          lane at the head of a run goes on;
//       b. the head adds its run to the slot of its label in a table in LDS: open addressing by a compare-and-swap on the key,
//          linear probing, at most PROBES slots tried, LDS atomics on the fields;
//       c. a head that found no slot (more labels in the tile than the table takes: a checkerboard has 4096) adds its run to the
//          region's entries in global memory itself: the fallback, complete on its own;
//       d. after a barrier every used slot is added to out[rank[label]] with one agent-scope atomic per field.
//     Global atomics per workgroup: fields x min(labels in the tile, TABLE) plus fields x the runs that overflowed -- not one per
//     pixel.  A constant mask costs one slot per workgroup.
//
// All sums in LDS are of tile-local coordinates (below 2^18) and of q <= 2^16 over at most 4096 pixels (2^28 at the most): int32.
// No workgroup waits for another anywhere: no flag, no spin, no grid barrier; every loop has a fixed trip count that the comment
// above it states.  Every accumulation is an integer add, min or max, so the result does not depend on any order.
#include <climits>

#include "gdl_common.h"
#include "infer_expr.h"
#include "../../include/gdlhip_scene_regions.h"

namespace {

#include "scan_u32.h"
#include "scene_common.h"
static_assert(SCAN_TILE == GDL_SCENE_REGIONS_SCAN_TILE, "the header states the scan's block size for the callers' scratch");

constexpr int TILE = GDL_SCENE_REGIONS_TILE;      // one wave per tile row: a lane is a column
constexpr int ROWS_PER_WAVE = TILE / 4;           // 256 threads = 4 waves
constexpr int TABLE = GDL_SCENE_REGIONS_TABLE;    // slots; ten int32 each: 40 KB of LDS, four workgroups per CU
constexpr int PROBES = GDL_SCENE_REGIONS_PROBES;
static_assert(TILE == 64 && (TABLE & (TABLE - 1)) == 0 && TABLE % 256 == 0 && PROBES >= 1 && PROBES <= TABLE, "a lane is a column");

// the arrays of gdl_scene_regions_stats; conf_sum / conf_min are looked at only where there is a canvas
struct RegionArrays {
  int32_t* label; uint8_t* value; int32_t* pixels; int32_t* bbox; int64_t* sum_xy; int64_t* conf_sum; int32_t* conf_min;
};

// what a set of pixels of one region adds to it: count, sums of x, y and q, minimum of q, box (x1, y1 exclusive)
struct Part {
  int n; int64_t sx, sy; int sq, mq, x0, y0, x1, y1;
};

// one global atomic per field into region r; r outside 0 .. N - 1 (labels that are not this mask's) is dropped
template <bool CONF>
__device__ __forceinline__ void add_global(const RegionArrays& out, int r, int N, const Part& p) {
  if ((unsigned)r >= (unsigned)N) return;
  __hip_atomic_fetch_add(out.pixels + r, p.n, RLX_AGENT);
  __hip_atomic_fetch_min(out.bbox + 4 * (int64_t)r + 0, p.x0, RLX_AGENT);
  __hip_atomic_fetch_min(out.bbox + 4 * (int64_t)r + 1, p.y0, RLX_AGENT);
  __hip_atomic_fetch_max(out.bbox + 4 * (int64_t)r + 2, p.x1, RLX_AGENT);
  __hip_atomic_fetch_max(out.bbox + 4 * (int64_t)r + 3, p.y1, RLX_AGENT);
  __hip_atomic_fetch_add(out.sum_xy + 2 * (int64_t)r + 0, p.sx, RLX_AGENT);
  __hip_atomic_fetch_add(out.sum_xy + 2 * (int64_t)r + 1, p.sy, RLX_AGENT);
  if constexpr (CONF) {
    __hip_atomic_fetch_add(out.conf_sum + r, (int64_t)p.sq, RLX_AGENT);
    __hip_atomic_fetch_min(out.conf_min + r, p.mq, RLX_AGENT);
  }
}

// ------------------------------------------------------------------ count
__global__ __launch_bounds__(256) void regions_roots_kernel(const int32_t* __restrict__ labels, int64_t HW, uint32_t* __restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) flag[i] = labels[i] == (int32_t)i;
}

// ------------------------------------------------------------------ fill
__global__ __launch_bounds__(256) void regions_fill_kernel(RegionArrays out, int N, int conf) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < N; r += (int64_t)gridDim.x * 256) {
    out.pixels[r] = 0;
    *(int4*)(out.bbox + 4 * r) = make_int4(INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN);
    out.sum_xy[2 * r] = 0;
    out.sum_xy[2 * r + 1] = 0;
    if (conf) { out.conf_sum[r] = 0; out.conf_min[r] = INT32_MAX; }
  }
}

// ------------------------------------------------------------------ statistics
// q of gdlhip_scene_regions.h for a pixel of value v.  The plane read for c is canvas[v] (canvas[0] for one class) where the
// canvas has one, otherwise the weight plane once more, whose value is then not used: canvas[v] and canvas[K] are the only
// planes touched, and along a row the reads are coalesced wherever v is constant.
__device__ __forceinline__ bool has_plane(int K, int v) { return K == 1 ? v <= 1 : v < K; }
__device__ __forceinline__ int class_plane(int K, int v) { return has_plane(K, v) ? (K == 1 ? 0 : v) : K; }
__device__ __forceinline__ int pixel_confidence(int K, int v, float c, float w) {
  float p = canvas_prob(c, w, w != 0.f);
  if (K == 1 && v == 0) p = 1.0f - p;
  return has_plane(K, v) && w != 0.f ? (int)rintf(p * 65536.0f) : 0;
}

template <bool CONF>
__global__ __launch_bounds__(256) void regions_stats_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ labels,
                                                            const int32_t* __restrict__ rank, const float* __restrict__ canvas, int K,
                                                            int H, int W, int tiles_x, int N, RegionArrays out) {
  // the table: t_key -1 = free.  Sums of tile-local x and y; boxes in tile-local coordinates, x1 / y1 inclusive here.
  __shared__ int t_key[TABLE], t_n[TABLE], t_sx[TABLE], t_sy[TABLE], t_sq[TABLE], t_mq[TABLE], t_x0[TABLE], t_x1[TABLE], t_y0[TABLE],
      t_y1[TABLE];
  const int lane = threadIdx.x & 63, row0 = (threadIdx.x >> 6) * ROWS_PER_WAVE;
  const int y0 = (int)(blockIdx.x / tiles_x) * TILE, x0 = (int)(blockIdx.x % tiles_x) * TILE;
  const int x = x0 + lane;
  const int64_t HW = (int64_t)H * W;

#pragma unroll
  for (int s = threadIdx.x; s < TABLE; s += 256) {      // TABLE / 256 turns
    t_key[s] = -1; t_n[s] = 0; t_sx[s] = 0; t_sy[s] = 0; t_x0[s] = TILE; t_x1[s] = -1; t_y0[s] = TILE; t_y1[s] = -1;
    if constexpr (CONF) { t_sq[s] = 0; t_mq[s] = INT32_MAX; }
  }

  // The wave's 16 rows: label (-1: ignored, outside the raster, or no index of this raster) and q.  The loads come in two
  // batches of independent ones -- labels, mask and weights of all rows, then the class planes the mask names -- so a thread
  // waits for memory twice, not three times per row; a position outside the raster reads the nearest pixel inside instead
  // (the last tile row and column alone), and what it reads is dropped.
  const int xc = x < W ? x : W - 1;
  int64_t at[ROWS_PER_WAVE];
  int lab[ROWS_PER_WAVE], val[ROWS_PER_WAVE], q[ROWS_PER_WAVE];
  [[maybe_unused]] float wgt[ROWS_PER_WAVE], cls[ROWS_PER_WAVE];
#pragma unroll
  for (int r = 0; r < ROWS_PER_WAVE; ++r) {      // ROWS_PER_WAVE turns
    const int y = y0 + row0 + r;
    at[r] = (int64_t)(y < H ? y : H - 1) * W + xc;
    lab[r] = labels[at[r]];
    val[r] = mask[at[r]];
    if constexpr (CONF) wgt[r] = canvas[(int64_t)K * HW + at[r]];
  }
  if constexpr (CONF) {
#pragma unroll
    for (int r = 0; r < ROWS_PER_WAVE; ++r) cls[r] = canvas[(int64_t)class_plane(K, val[r]) * HW + at[r]];      // ROWS_PER_WAVE turns
  }
#pragma unroll
  for (int r = 0; r < ROWS_PER_WAVE; ++r) {      // ROWS_PER_WAVE turns
    const bool in = y0 + row0 + r < H && x < W && (unsigned)lab[r] < (unsigned)HW;
    q[r] = 0;
    if constexpr (CONF) q[r] = in ? pixel_confidence(K, val[r], cls[r], wgt[r]) : 0;
    if (in && lab[r] == (int)at[r]) {      // the root pixel names its region: one thread of the grid per region
      const int n = rank[at[r]];
      if ((unsigned)n < (unsigned)N) { out.label[n] = lab[r]; out.value[n] = (uint8_t)val[r]; }
    }
    lab[r] = in ? lab[r] : -1;
  }
  __syncthreads();      // the table is cleared

#pragma unroll
  for (int r = 0; r < ROWS_PER_WAVE; ++r) {      // ROWS_PER_WAVE turns
    const int ly = row0 + r, l = lab[r];
    const int left = __shfl_up(l, 1, 64);
    const unsigned long long m = __ballot(lane == 0 || l != left);       // bit 0 is always set
    if (m == 1ull && l < 0) continue;                                    // wave-uniform: nothing in this row
    const int start = 63 - __clzll(m & (~0ull >> (63 - lane)));          // the last start at or before this lane
    const unsigned long long after = lane == 63 ? 0ull : m >> (lane + 1) << (lane + 1);
    const int end = after ? __ffsll((long long)after) - 2 : 63;          // the lane before the next start
    int sq = q[r], mq = q[r];
    if constexpr (CONF) {
      // segmented scan towards the head: after the step of o, a lane holds its run's lanes lane .. min(lane + 2 o - 1, end)
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {      // 6 turns
        const int s2 = __shfl_down(sq, o, 64), m2 = __shfl_down(mq, o, 64);
        if (lane + o <= end) { sq += s2; mq = m2 < mq ? m2 : mq; }
      }
    }
    if (lane != start || l < 0) continue;
    const int n = end - start + 1, sx = (start + end) * n / 2;      // the run is the lanes start .. end of row ly
    bool placed = false;
    unsigned s = ((unsigned)l * 2654435761u) >> 16;
    for (int t = 0; t < PROBES && !placed; ++t, ++s) {      // at most PROBES turns
      const int slot = (int)(s & (TABLE - 1));
      const int k = atomicCAS(&t_key[slot], -1, l);
      if (k != -1 && k != l) continue;
      placed = true;
      atomicAdd(&t_n[slot], n);
      atomicAdd(&t_sx[slot], sx);
      atomicAdd(&t_sy[slot], ly * n);
      atomicMin(&t_x0[slot], start);
      atomicMax(&t_x1[slot], end);
      atomicMin(&t_y0[slot], ly);
      atomicMax(&t_y1[slot], ly);
      if constexpr (CONF) { atomicAdd(&t_sq[slot], sq); atomicMin(&t_mq[slot], mq); }
    }
    if (!placed) {
      const int64_t gx = x0, gy = y0 + ly;
      add_global<CONF>(out, rank[l], N, Part{n, sx + gx * n, gy * n, sq, mq, x0 + start, y0 + ly, x0 + end + 1, y0 + ly + 1});
    }
  }
  __syncthreads();

#pragma unroll
  for (int s = threadIdx.x; s < TABLE; s += 256) {      // TABLE / 256 turns
    const int l = t_key[s];
    if (l < 0) continue;
    const int n = t_n[s];
    const int64_t gx = x0, gy = y0;
    add_global<CONF>(out, rank[l], N, Part{n, t_sx[s] + gx * n, t_sy[s] + gy * n, CONF ? t_sq[s] : 0, CONF ? t_mq[s] : 0, x0 + t_x0[s],
                                           y0 + t_y0[s], x0 + t_x1[s] + 1, y0 + t_y1[s] + 1});
  }
}

}  // namespace

extern "C" int gdl_scene_regions_count(const int32_t* labels, int H, int W, int32_t* rank, int32_t* block_sums, int32_t* n_regions,
                                       gdl_stream_t stream) {
  GDL_CHECK_ARG(labels && rank && block_sums && n_regions, "gdl_scene_regions_count: null pointer");
  if (const int bad = check_raster("gdl_scene_regions_count", H, W, LINEAR_INDEX)) return bad;
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  hipLaunchKernelGGL(regions_roots_kernel, dim3(grid_for(HW)), dim3(256), 0, s, labels, HW, (uint32_t*)rank);
  scan_exclusive((uint32_t*)rank, 1, HW, (uint32_t*)block_sums, (uint32_t*)n_regions, s);
  GDL_CHECK_LAUNCH("gdl_scene_regions_count");
  return GDL_OK;
}

extern "C" int gdl_scene_regions_stats(const uint8_t* mask, const int32_t* labels, const int32_t* rank, const float* canvas, int K, int H,
                                       int W, int N, int32_t* label, uint8_t* value, int32_t* pixels, int32_t* bbox, int64_t* sum_xy,
                                       int64_t* conf_sum, int32_t* conf_min, gdl_stream_t stream) {
  if (const int bad = check_raster("gdl_scene_regions_stats", H, W, LINEAR_INDEX)) return bad;
  GDL_CHECK_ARG(N >= 0 && N <= (int64_t)H * W, "gdl_scene_regions_stats: %d regions in %d x %d pixels", N, H, W);
  if (N == 0) return GDL_OK;
  GDL_CHECK_ARG(mask && labels && rank && label && value && pixels && bbox && sum_xy && (!canvas || (conf_sum && conf_min)),
                "gdl_scene_regions_stats: null pointer");
  GDL_CHECK_ARG(!canvas || (K >= 1 && K <= 255), "gdl_scene_regions_stats: 1..255 classes, got %d", K);
  GDL_CHECK_ARG((uintptr_t)bbox % 16 == 0, "gdl_scene_regions_stats: bbox must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const RegionArrays out{label, value, pixels, bbox, sum_xy, conf_sum, conf_min};
  hipLaunchKernelGGL(regions_fill_kernel, dim3(grid_for(N)), dim3(256), 0, s, out, N, canvas != nullptr);
  const int tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE;
  const dim3 tiles((unsigned)(tiles_x * tiles_y));      // at most 2^31 / 4096 + the partial ones
  if (canvas) hipLaunchKernelGGL(regions_stats_kernel<true>, tiles, dim3(256), 0, s, mask, labels, rank, canvas, K, H, W, tiles_x, N, out);
  else hipLaunchKernelGGL(regions_stats_kernel<false>, tiles, dim3(256), 0, s, mask, labels, rank, canvas, 0, H, W, tiles_x, N, out);
  GDL_CHECK_LAUNCH("gdl_scene_regions_stats");
  return GDL_OK;
}
