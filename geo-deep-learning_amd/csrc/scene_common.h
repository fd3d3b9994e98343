// What the vector stages of whole-scene inference share (scene_sieve / scene_rings / scene_simplify / scene_regions /
// scene_burn.hip): the small helpers, the rule that says which pixels of a mask are live, and the argument checks of a raster.
// No kernel lives here.  Include inside the file's anonymous namespace, after gdl_common.h, like scan_u32.h.
#pragma once

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// Every index that a kernel reads from memory and then uses as an address is held against the array's size first: the arrays
// are the caller's, and a gather must stay inside them even where they were not filled by the calls before.
__device__ __forceinline__ bool in_range(int i, int n) { return (unsigned)i < (unsigned)n; }

inline dim3 one_per_thread(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }      // n <= 2^31: at most 2^23 workgroups

// ------------------------------------------------------------------ the live rule
// A pixel is live when it is not `ignore_label` and keep[its value] is set.  gdl_scene_rings_* and gdl_scene_nodes both read
// the mask through this struct alone, which is what makes the nodes those of the rings.
struct Raster {
  const uint8_t* __restrict__ mask;
  const uint8_t* __restrict__ keep;
  int H, W, ignore_label;
  __device__ __forceinline__ bool inside(int y, int x) const { return y >= 0 && y < H && x >= 0 && x < W; }
  // the value of pixel (y, x) of the raster where it is live, otherwise -1
  __device__ __forceinline__ int live(int y, int x) const {
    const int v = mask[(int64_t)y * W + x];
    return v != ignore_label && keep[v] ? v : -1;
  }
  // the same for any cell of the plane: -1 outside the raster too
  __device__ __forceinline__ int cell(int y, int x) const { return inside(y, x) ? live(y, x) : -1; }
};

// ------------------------------------------------------------------ the checks of a raster's arguments
// H * W must stay below what the stage indexes with, and the message says which index that is
struct PixelLimit {
  int64_t below;
  const char* why;
};
constexpr PixelLimit LINEAR_INDEX{(int64_t)1 << 31, "a linear index must fit an int32 (H * W < 2^31)"};
constexpr PixelLimit RING_SLOT{(int64_t)1 << 29, "a slot 4 * (y * W + x) + side must fit an int32 (H * W < 2^29)"};
constexpr PixelLimit RING_RASTER{(int64_t)1 << 29, "the rings are those of a raster of H * W < 2^29"};

int check_raster(const char* fn, int H, int W, const PixelLimit& limit) {
  GDL_CHECK_ARG(H > 0 && W > 0, "%s: bad sizes", fn);
  GDL_CHECK_ARG((int64_t)H * W < limit.below, "%s: %d x %d pixels: %s", fn, H, W, limit.why);
  return GDL_OK;
}

int check_connectivity(const char* fn, int connectivity) {
  GDL_CHECK_ARG(connectivity == 4 || connectivity == 8, "%s: connectivity %d is neither 4 nor 8", fn, connectivity);
  return GDL_OK;
}

int check_ignore_label(const char* fn, int ignore_label) {
  GDL_CHECK_ARG(ignore_label >= -1 && ignore_label <= 255, "%s: ignore_label %d is not in -1..255", fn, ignore_label);
  return GDL_OK;
}
