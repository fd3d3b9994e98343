// Sieve of a label mask (include/gdlhip_scene_sieve.h): connected components by union-find, then the dissolving of the small ones.
//
// The parents of the union-find live in `labels`: parent[i] <= i on every pixel of a component, parent[i] == i at a root, -1 on an
// ignored pixel.  A union always hangs the root with the larger index under the one with the smaller, so the root of a finished
// component is its smallest linear index, which is the label asked for.  Three launches, each seeing the stores of the one before
// through the kernel boundary:
//   1. components_tile_kernel: one workgroup per TILE x TILE pixels, the union-find of the tile alone in LDS, written out as global
//      indices (every pixel points straight at its tile's root);
//   2. components_border_kernel: one thread per pixel on a tile edge, the unions across the edge.  Workgroups on every XCD work on
//      the same parents at once here, so every access to them in this kernel is an agent-scope atomic;
//   3. components_flatten_kernel: one workgroup per tile, labels[i] = root(i) and the pixel counts, added up per tile in LDS first.
//
// No workgroup waits for another anywhere: there is no flag, no spin and no grid barrier, and every loop is bounded by an index
// that strictly decreases (the comment above each loop says which).
#include "gdl_common.h"
#include "../../include/gdlhip_scene_sieve.h"

namespace {

#include "scene_common.h"

constexpr int TILE = 64;                 // one wave per tile row: a lane is a column.  64 x 64 int32 parents are 16 KB of LDS
constexpr int TILE_PIXELS = TILE * TILE;
constexpr int ROWS_PER_WAVE = TILE / 4;  // 256 threads = 4 waves

// ------------------------------------------------------------------ union-find
// find and unite over one parent array, SCOPE telling who else works on it: the workgroup (LDS) or the whole device.
// Invariant: parent[i] <= i, and an entry only ever decreases.
template <int SCOPE>
struct UnionFind {
  int* parent;
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, SCOPE); }
  // Ends: x takes the value parent[x] < x each turn, and indices are >= 0.  An entry read a moment before another thread lowers it
  // is still an ancestor, so a stale read costs a step and never leaves the component.
  __device__ __forceinline__ int find(int x) const {
    for (int p = load(x); p != x; p = load(x)) x = p;
    return x;
  }
  // Ends: each turn either leaves or replaces a = max(a, b) by old < a, so a + b strictly decreases and is >= 0; nothing in it
  // waits for a value another thread has yet to write.  When the atomic minimum finds parent[a] == old != a, the entry holds
  // min(old, b) afterwards and the union that is still owed is the one of old and b: whichever of the two the entry dropped,
  // this thread goes on to join it.
  __device__ __forceinline__ void unite(int a, int b) const {
    a = find(a);
    b = find(b);
    while (a != b) {
      if (a < b) { const int t = a; a = b; b = t; }
      const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, SCOPE);
      if (old == a) break;      // a was a root and now hangs under b
      a = old;
    }
  }
};

// ------------------------------------------------------------------ 1. the tile's own components, in LDS
// Thread (wave w, lane x) owns column x of rows w * 16 .. w * 16 + 15 of the tile.  s_val: the pixel's value, -1 where it is
// ignored or outside the raster, so that equal and >= 0 means "one component".
//   a. row runs: a ballot marks where a run starts, and every pixel points at the start of its run: a run costs no union at all;
//   b. the unions with the row above.  The one straight up is left out where the pair to the left is joined as well (the two
//      runs already meet there); the two diagonal ones (connectivity 8) are left out where the pixel straight up joins anyway;
//   c. every pixel looks its root up and writes it as a global index; sizes is zeroed on the way for launch 3.
__global__ __launch_bounds__(256) void components_tile_kernel(const uint8_t* __restrict__ mask, int H, int W, int tiles_x, int conn8,
                                                              int ignore_label, int32_t* __restrict__ parent, int32_t* __restrict__ sizes) {
  __shared__ int s_parent[TILE_PIXELS];
  __shared__ int16_t s_val[TILE_PIXELS];
  const int lane = threadIdx.x & 63, row0 = (threadIdx.x >> 6) * ROWS_PER_WAVE;
  const int y0 = (int)(blockIdx.x / tiles_x) * TILE, x0 = (int)(blockIdx.x % tiles_x) * TILE;
  const int x = x0 + lane;
  const UnionFind<__HIP_MEMORY_SCOPE_WORKGROUP> uf{s_parent};

  for (int r = 0; r < ROWS_PER_WAVE; ++r) {
    const int ly = row0 + r, y = y0 + ly;
    int v = -1;
    if (y < H && x < W) {
      v = mask[(int64_t)y * W + x];
      if (v == ignore_label) v = -1;
    }
    const int left = __shfl_up(v, 1, 64);
    const bool starts = lane == 0 || v < 0 || v != left;
    const unsigned long long m = __ballot(starts);                       // bit 0 is always set
    const int start = 63 - __clzll(m & (~0ull >> (63 - lane)));          // the last start at or before this lane
    s_val[ly * TILE + lane] = (int16_t)v;
    s_parent[ly * TILE + lane] = ly * TILE + start;
  }
  __syncthreads();

  for (int r = 0; r < ROWS_PER_WAVE; ++r) {
    const int ly = row0 + r, i = ly * TILE + lane;
    const int v = s_val[i];
    if (ly == 0 || v < 0) continue;
    const int up = i - TILE;
    const bool up_same = s_val[up] == v;
    if (up_same) {
      if (!(lane > 0 && s_val[i - 1] == v && s_val[up - 1] == v)) uf.unite(i, up);
    } else if (conn8) {
      if (lane > 0 && s_val[up - 1] == v) uf.unite(i, up - 1);
      if (lane < TILE - 1 && s_val[up + 1] == v) uf.unite(i, up + 1);
    }
  }
  __syncthreads();

  for (int r = 0; r < ROWS_PER_WAVE; ++r) {
    const int ly = row0 + r, y = y0 + ly;
    if (y >= H || x >= W) continue;
    const int i = ly * TILE + lane;
    const int64_t g = (int64_t)y * W + x;
    int root = -1;
    if (s_val[i] >= 0) {
      const int l = uf.find(i);
      root = (y0 + l / TILE) * W + x0 + l % TILE;      // the order of the local indices is the order of the global ones
    }
    parent[g] = root;
    sizes[g] = 0;
  }
}

// ------------------------------------------------------------------ 2. the unions across the tile edges
// Item t < n_h is pixel (y, x) of the first row of a tile row below the first: y = (t / W + 1) * TILE.  Its partners are the pixel
// straight up and, for connectivity 8 where that one does not join anyway, the two diagonally up.  The remaining items are the
// pixels of the first column of a tile column: x = (t' / H + 1) * TILE, partners to the left and diagonally left (up and down).
// A pair across a corner is met from both sides, which a union does not mind.  As in the tile kernel, the straight union is left
// out where its neighbour pair one step back along the edge is joined too and both steps stay inside their tiles: a constant
// mask then costs one union per tile edge, not one per edge pixel, on the one address all of them would otherwise fight for.
//
// The mask is the launch's input and is read plainly.  `parent` is read and written by workgroups on every XCD at once, whose
// L2s are not coherent with each other and whose L1s are never refreshed: it is touched through UnionFind<agent> alone, whose
// loads and minima are agent-scope atomics (served where all XCDs meet).  Nobody polls: a thread's unions end by themselves
// (UnionFind), and the components are complete when the launch is, whatever the order.
__global__ __launch_bounds__(256) void components_border_kernel(const uint8_t* __restrict__ mask, int H, int W, int conn8, int ignore_label,
                                                                int32_t* parent, int64_t n_h, int64_t n_items) {
  const UnionFind<__HIP_MEMORY_SCOPE_AGENT> uf{parent};
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_items; t += (int64_t)gridDim.x * 256) {
    int y, x;
    const bool dx = t < n_h;      // the edge runs along x (a tile row's first row) or along y (a tile column's first column)
    if (dx) { y = (int)(t / W + 1) * TILE; x = (int)(t % W); }
    else { const int64_t u = t - n_h; x = (int)(u / H + 1) * TILE; y = (int)(u % H); }
    const int i = y * W + x;                 // H * W < 2^31
    const int v = mask[i];
    if (v == ignore_label) continue;
    const int across = dx ? -W : -1;         // to the partner straight across the edge
    const int along = dx ? 1 : W;
    const int pos = dx ? x : y, len = dx ? W : H;
    if (mask[i + across] == v) {
      const bool back_joined = pos % TILE != 0 && mask[i - along] == v && mask[i + across - along] == v;
      if (!back_joined) uf.unite(i, i + across);
    } else if (conn8) {
      if (pos > 0 && mask[i + across - along] == v) uf.unite(i, i + across - along);
      if (pos < len - 1 && mask[i + across + along] == v) uf.unite(i, i + across + along);
    }
  }
}

// ------------------------------------------------------------------ 3. labels and sizes
// One workgroup per tile again.  A pixel is counted in LDS under a slot of its own tile: the pixel its parent names where that one
// lies in the tile (launch 1 left every pixel pointing at its tile's root, and launch 2 rewrote the entries of such roots alone),
// otherwise itself.  Whatever launch 2 did, a slot's pixel lies in the component of every pixel counted under it, so one find and
// one global add per used slot -- per component of the tile, not per pixel -- give exact sizes, and the root found is the label
// of all the slot's pixels.
//
// `parent` is `labels`: the flattening is in place.  An entry is written by its own tile's workgroup alone, after that workgroup
// has read it; a find of another workgroup that passes through reads the entry of launch 2 or the root, and either leads to
// the same root.  The finds read with agent-scope atomic loads so that nothing is assumed about which of the two they see.
__global__ __launch_bounds__(256) void components_flatten_kernel(int H, int W, int tiles_x, int32_t* parent, int32_t* __restrict__ sizes) {
  __shared__ int s_count[TILE_PIXELS];
  const int lane = threadIdx.x & 63, row0 = (threadIdx.x >> 6) * ROWS_PER_WAVE;
  const int y0 = (int)(blockIdx.x / tiles_x) * TILE, x0 = (int)(blockIdx.x % tiles_x) * TILE;
  const int x = x0 + lane;
  const UnionFind<__HIP_MEMORY_SCOPE_AGENT> uf{parent};
  for (int i = threadIdx.x; i < TILE_PIXELS; i += 256) s_count[i] = 0;
  __syncthreads();

  int slot[ROWS_PER_WAVE];      // -1: nothing to count (ignored, or outside the raster)
#pragma unroll
  for (int r = 0; r < ROWS_PER_WAVE; ++r) {
    const int ly = row0 + r, y = y0 + ly;
    slot[r] = -1;
    if (y < H && x < W) {
      const int p = parent[(int64_t)y * W + x];
      if (p >= 0) {
        const int py = p / W - y0, px = p % W - x0;
        slot[r] = py >= 0 && py < TILE && px >= 0 && px < TILE ? py * TILE + px : ly * TILE + lane;
      }
    }
    // the lanes that share the first counted lane's slot -- as a rule the whole row -- add once
    const unsigned long long counted = __ballot(slot[r] >= 0);
    if (counted) {
      const int lead = __ffsll((long long)counted) - 1;
      const int s0 = __shfl(slot[r], lead, 64);
      const unsigned long long same = __ballot(slot[r] == s0);
      if (lane == lead) atomicAdd(&s_count[s0], __popcll(same));
      else if (slot[r] >= 0 && slot[r] != s0) atomicAdd(&s_count[slot[r]], 1);
    }
  }
  __syncthreads();

  for (int i = threadIdx.x; i < TILE_PIXELS; i += 256) {
    const int n = s_count[i];
    if (n > 0) {
      const int root = uf.find((y0 + i / TILE) * W + x0 + i % TILE);
      __hip_atomic_fetch_add(sizes + root, n, RLX_AGENT);
      s_count[i] = root;
    }
  }
  __syncthreads();

#pragma unroll
  for (int r = 0; r < ROWS_PER_WAVE; ++r) {
    const int y = y0 + row0 + r;
    if (y < H && x < W) parent[(int64_t)y * W + x] = slot[r] >= 0 ? s_count[slot[r]] : -1;
  }
}

// ------------------------------------------------------------------ the sieve
// whether pixel i belongs to a small component, and that component's root
__device__ __forceinline__ bool small_root(const int32_t* __restrict__ labels, const int32_t* __restrict__ sizes, int64_t i, int min_size,
                                           int& root) {
  root = labels[i];
  return root >= 0 && sizes[root] < min_size;
}

// best[root] = 0 at the root of every small component: the only entries the two kernels below look at
__global__ __launch_bounds__(256) void sieve_clear_kernel(const int32_t* __restrict__ sizes, int64_t HW, int min_size, int64_t* __restrict__ best) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
    const int n = sizes[i];
    if (n > 0 && n < min_size) best[i] = 0;
  }
}

// A pixel of a small component offers the key of every kept component among its neighbours to its root: a maximum, whose result
// does not depend on the order of the offers.  The size is at most 2^31 - 1, so the key is below 2^39 and positive.
__global__ __launch_bounds__(256) void sieve_vote_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ sizes, int H, int W, int conn8, int min_size,
                                                         int64_t* best) {
  const int64_t HW = (int64_t)H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
    int root;
    if (!small_root(labels, sizes, i, min_size, root)) continue;
    const int y = (int)(i / W), x = (int)(i % W);
    int64_t key = 0;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if ((dy == 0 && dx == 0) || (!conn8 && dy != 0 && dx != 0)) continue;
        const int ny = y + dy, nx = x + dx;
        if (ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
        const int64_t j = (int64_t)ny * W + nx;
        const int other = labels[j];
        if (other < 0 || other == root) continue;
        const int n = sizes[other];
        if (n < min_size) continue;
        const int64_t k = ((int64_t)n << 8) | (255 - mask[j]);
        key = k > key ? k : key;
      }
    if (key) __hip_atomic_fetch_max(best + root, key, RLX_AGENT);
  }
}

__global__ __launch_bounds__(256) void sieve_apply_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ sizes, int64_t HW, int min_size,
                                                          const int64_t* __restrict__ best, uint8_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
    int root;
    uint8_t v = mask[i];
    if (small_root(labels, sizes, i, min_size, root)) {
      const int64_t key = best[root];
      if (key) v = (uint8_t)(255 - (int)(key & 255));
    }
    out[i] = v;
  }
}

int check_common(const char* fn, int H, int W, int connectivity, int ignore_label) {
  if (const int bad = check_raster(fn, H, W, LINEAR_INDEX)) return bad;
  if (const int bad = check_connectivity(fn, connectivity)) return bad;
  return check_ignore_label(fn, ignore_label);
}

}  // namespace

extern "C" int gdl_scene_components(const uint8_t* mask, int H, int W, int connectivity, int ignore_label, int32_t* labels, int32_t* sizes,
                                    gdl_stream_t stream) {
  GDL_CHECK_ARG(mask && labels && sizes, "gdl_scene_components: null pointer");
  if (const int bad = check_common("gdl_scene_components", H, W, connectivity, ignore_label)) return bad;
  hipStream_t s = (hipStream_t)stream;
  const int tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE, conn8 = connectivity == 8;
  const dim3 tiles((unsigned)(tiles_x * tiles_y));      // at most 2^31 / 4096 + the partial ones
  hipLaunchKernelGGL(components_tile_kernel, tiles, dim3(256), 0, s, mask, H, W, tiles_x, conn8, ignore_label, labels, sizes);
  const int64_t n_h = (int64_t)(tiles_y - 1) * W, n_items = n_h + (int64_t)(tiles_x - 1) * H;
  if (n_items > 0)
    hipLaunchKernelGGL(components_border_kernel, dim3(grid_for(n_items)), dim3(256), 0, s, mask, H, W, conn8, ignore_label, labels, n_h, n_items);
  hipLaunchKernelGGL(components_flatten_kernel, tiles, dim3(256), 0, s, H, W, tiles_x, labels, sizes);
  GDL_CHECK_LAUNCH("gdl_scene_components");
  return GDL_OK;
}

extern "C" int gdl_scene_sieve(const uint8_t* mask, const int32_t* labels, const int32_t* sizes, int H, int W, int connectivity,
                               int min_size, int ignore_label, int64_t* best, uint8_t* out, gdl_stream_t stream) {
  GDL_CHECK_ARG(mask && labels && sizes && best && out, "gdl_scene_sieve: null pointer");
  if (const int bad = check_common("gdl_scene_sieve", H, W, connectivity, ignore_label)) return bad;
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const dim3 grid(grid_for(HW));
  if (min_size > 1) {      // otherwise no component is small and the last kernel copies the mask
    hipLaunchKernelGGL(sieve_clear_kernel, grid, dim3(256), 0, s, sizes, HW, min_size, best);
    hipLaunchKernelGGL(sieve_vote_kernel, grid, dim3(256), 0, s, mask, labels, sizes, H, W, connectivity == 8, min_size, best);
  }
  hipLaunchKernelGGL(sieve_apply_kernel, grid, dim3(256), 0, s, mask, labels, sizes, HW, min_size, (const int64_t*)best, out);
  GDL_CHECK_LAUNCH("gdl_scene_sieve");
  return GDL_OK;
}
