// Whole-scene inference (include/gdlhip_scene.h): cut normalised tiles out of a raster, stitch the tiles' class probabilities into a
// weighted canvas, label the canvas.  All four kernels are bound by memory traffic; none uses atomics, so every result is
// reproducible bit for bit.  Test-time augmentation (include/gdlhip_scene_tta.h) is the same cut and blend kernels with a D4 code
// per tile in the index arithmetic of their gathers: a flag of the cut kernel, two further sources of the blend kernel.  Nodata
// (include/gdlhip_scene_nodata.h) is a validity plane of the raster: one kernel builds it, one counts it per tile, and the cut and
// the finish kernels read it under one more flag each.
#include <cmath>

#include "gdl_common.h"
#include "bilinear_index.h"
#include "infer_expr.h"
#include "../../include/gdlhip_scene.h"
#include "../../include/gdlhip_scene_tta.h"
#include "../../include/gdlhip_scene_nodata.h"

namespace {

// ------------------------------------------------------------------ D4 transform codes (include/gdlhip_scene_tta.h)
// T_g(x)[i][j] = x[r][c] for a result of rows x cols (square where g & 4): flip, then swap.  With g in 0..7 (0..3 for a tile that
// is not square) r stays inside 0..rows-1 and c inside 0..cols-1 of x.
__device__ __forceinline__ void d4_src(int g, int rows, int cols, int i, int j, int& r, int& c) {
  const int a = g & 2 ? rows - 1 - i : i, b = g & 1 ? cols - 1 - j : j;
  r = g & 4 ? b : a;
  c = g & 4 ? a : b;
}

// the code of tile t as the kernels take it: whatever the array holds, no code transposes a tile that is not square
__device__ __forceinline__ int d4_code(const int32_t* __restrict__ xforms, int t, int th, int tw) { return xforms[t] & (th == tw ? 7 : 3); }

__device__ __forceinline__ int d4_inverse(int g) { return g & 4 ? 4 | (g & 1) << 1 | (g >> 1 & 1) : g; }

// ------------------------------------------------------------------ cut
// A thread writes V consecutive values of one tile row (V == 4: one 16-byte store, tw % 4 == 0); the raster is read element by
// element because a tile origin has no alignment.  The value is normalize_range_value of infer_expr.h, the function
// normalize_range_kernel evaluates, on the raw sample or, outside the raster, on `fill`.
//
// D4 (include/gdlhip_scene_tta.h): the tile written is T_g of the tile cut, g = xforms[b].  The stores stay what they are; the V
// raster elements of a thread lie along a row (backwards where g flips x) or, under a transpose, down a column.
//
// MASKED (include/gdlhip_scene_nodata.h): a pixel inside the raster whose valid[y, x] is 0 takes `fill` as well; one more byte read
// per element, the same for every band.  Without the flag `valid` is not looked at.
template <typename TI, int V, bool D4, bool MASKED>
__global__ __launch_bounds__(256) void scene_cut_kernel(const TI* __restrict__ raster, int C, int H, int W,
                                                        const int32_t* __restrict__ origins, const int32_t* __restrict__ xforms, int th,
                                                        int tw, float fill, float* __restrict__ tiles, int64_t groups, float imin,
                                                        float span, float d, float nmin, const float* __restrict__ mean,
                                                        const float* __restrict__ stdv, const uint8_t* __restrict__ valid) {
  struct alignas(sizeof(float) * V) VecF { float v[V]; };
  const int twv = tw / V;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int dx0 = (int)(g % twv) * V;
    int64_t t = g / twv;
    const int dy = (int)(t % th);
    t /= th;
    const int c = (int)(t % C), b = (int)(t / C);
    const float m = mean[c], s = stdv[c];
    VecF o;
    if constexpr (D4) {
      const int code = d4_code(xforms, b, th, tw);
      const int64_t oy = origins[2 * b], ox = origins[2 * b + 1];
      const TI* plane = raster + (int64_t)c * H * W;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        int r, q;
        d4_src(code, th, tw, dy, dx0 + e, r, q);
        const int64_t y = oy + r, x = ox + q;
        bool in = y >= 0 && y < H && x >= 0 && x < W;
        if constexpr (MASKED) in = in && valid[y * W + x] != 0;
        const float raw = in ? (float)plane[y * W + x] : fill;
        o.v[e] = normalize_range_value(raw, imin, span, d, nmin, m, s);
      }
    } else {
      const int64_t y = (int64_t)origins[2 * b] + dy, x0 = (int64_t)origins[2 * b + 1] + dx0;
      const bool row_in = y >= 0 && y < H;
      const TI* row = raster + ((int64_t)c * H + (row_in ? y : 0)) * W;
      const uint8_t* vrow = MASKED ? valid + (row_in ? y : 0) * W : nullptr;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int64_t x = x0 + e;
        bool in = row_in && x >= 0 && x < W;
        if constexpr (MASKED) in = in && vrow[x] != 0;
        const float raw = in ? (float)row[x] : fill;
        o.v[e] = normalize_range_value(raw, imin, span, d, nmin, m, s);
      }
    }
    *(VecF*)(tiles + g * V) = o;
  }
}

// ------------------------------------------------------------------ blend
// Where the class probabilities of tile pixel (dy, dx0 + e), e < V, come from.  `cov[e]` says which of the V pixels the tile covers;
// only those are read and only their p[e] is defined.

// the tiles' full-resolution probabilities [B, K, th, tw]
template <int K>
struct ProbsSource {
  const float* probs;
  int th, tw;
  bool vec;   // tw % 4 == 0 and a 16-byte aligned base: four covered pixels at dx0 % 4 == 0 are one 16-byte load per class
  __device__ __forceinline__ void prepare() {}
  template <int V>
  __device__ __forceinline__ void load(int t, int dy, int dx0, const bool (&cov)[V], float (&p)[V][K]) const {
    const float* base = probs + (((int64_t)t * K) * th + dy) * tw + dx0;
    const int64_t plane = (int64_t)th * tw;
    if constexpr (V == 4) {
      if (vec && (dx0 & 3) == 0 && cov[0] && cov[1] && cov[2] && cov[3]) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float4 q = *(const float4*)(base + k * plane);
          p[0][k] = q.x; p[1][k] = q.y; p[2][k] = q.z; p[3][k] = q.w;
        }
        return;
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (cov[e]) {
#pragma unroll
        for (int k = 0; k < K; ++k) p[e][k] = base[k * plane + e];
      }
  }
};

// a head's own map [B, hi, wi, K] (NHWC): the pixel's probabilities as upsample_probs_kernel evaluates them -- src_index2 and
// bilinear_logits of bilinear_index.h, logits_to_probs of infer_expr.h, the ratios formed on the device as that kernel forms them
template <int K>
struct LowresSource {
  const float* low;
  int hi, wi, th, tw;
  float ry, rx;
  __device__ __forceinline__ void prepare() { ry = (float)hi / (float)th; rx = (float)wi / (float)tw; }
  template <int V>
  __device__ __forceinline__ void load(int t, int dy, int dx0, const bool (&cov)[V], float (&p)[V][K]) const {
    int y0, y1; float ly;
    src_index2(ry, dy, hi, y0, y1, ly);
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (cov[e]) {
        int x0, x1; float lx;
        src_index2(rx, dx0 + e, wi, x0, x1, lx);
        bilinear_logits<K>(low, t, hi, wi, y0, y1, x0, x1, ly, lx, p[e]);
        logits_to_probs<K>(p[e]);
      }
  }
};

// The two sources with a D4 code per tile: the tile's values are in the transformed frame, so tile-frame pixel (dy, dx) of the
// canvas reads T_g^-1(.)[dy][dx] = d4_src with the inverse code.  The kernel, its canvas accesses and the weight wy[dy] * wx[dx]
// are untouched.  The tile index is the same in every lane of a workgroup, so the branches on the code do not diverge.
template <int K>
struct ProbsSourceD4 {
  const float* probs;
  const int32_t* xforms;
  int th, tw;
  bool vec;   // as in ProbsSource
  __device__ __forceinline__ void prepare() {}
  template <int V>
  __device__ __forceinline__ void load(int t, int dy, int dx0, const bool (&cov)[V], float (&p)[V][K]) const {
    const int g = d4_inverse(d4_code(xforms, t, th, tw));
    const int64_t plane = (int64_t)th * tw;
    const float* tile = probs + (int64_t)t * K * plane;
    if constexpr (V == 4) {
      // without a transpose the four pixels are four neighbours of one tile row, ascending or (flip x) descending: tw % 4 == 0
      // and dx0 % 4 == 0 make tw - 4 - dx0 a multiple of four as well, so either way it is one 16-byte load per class
      if (!(g & 4) && vec && (dx0 & 3) == 0 && cov[0] && cov[1] && cov[2] && cov[3]) {
        const bool rev = g & 1;
        const float* base = tile + (int64_t)(g & 2 ? th - 1 - dy : dy) * tw + (rev ? tw - 4 - dx0 : dx0);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float4 q = *(const float4*)(base + k * plane);
          p[0][k] = rev ? q.w : q.x; p[1][k] = rev ? q.z : q.y; p[2][k] = rev ? q.y : q.z; p[3][k] = rev ? q.x : q.w;
        }
        return;
      }
    }
    // under a transpose the four pixels read a column of the tile: one load per element
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (cov[e]) {
        int r, c;
        d4_src(g, th, tw, dy, dx0 + e, r, c);
        const float* base = tile + (int64_t)r * tw + c;
#pragma unroll
        for (int k = 0; k < K; ++k) p[e][k] = base[k * plane];
      }
  }
};

template <int K>
struct LowresSourceD4 {
  const float* low;
  const int32_t* xforms;
  int hi, wi, th, tw;
  float ry, rx;
  __device__ __forceinline__ void prepare() { ry = (float)hi / (float)th; rx = (float)wi / (float)tw; }
  template <int V>
  __device__ __forceinline__ void load(int t, int dy, int dx0, const bool (&cov)[V], float (&p)[V][K]) const {
    const int g = d4_inverse(d4_code(xforms, t, th, tw));
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (cov[e]) {
        int r, c, y0, y1, x0, x1; float ly, lx;
        d4_src(g, th, tw, dy, dx0 + e, r, c);      // where the pixel lies in the transformed tile, whose map `low` is
        src_index2(ry, r, hi, y0, y1, ly);
        src_index2(rx, c, wi, x0, x1, lx);
        bilinear_logits<K>(low, t, hi, wi, y0, y1, x0, x1, ly, lx, p[e]);
        logits_to_probs<K>(p[e]);
      }
  }
};

constexpr int PATCH_W = 64;   // canvas columns of one workgroup's patch; its rows: 256 threads / (PATCH_W / V) = 16 (V == 4) or 4 (V == 1)

// One workgroup per patch of the batch's bounding box, one thread per V consecutive canvas pixels of a row (V == 4: W % 4 == 0 and
// a 16-byte aligned canvas, so every plane is read and written with 16-byte accesses along W; V == 1 otherwise).  The tiles of the
// batch are taken 256 at a time: thread i tests tile base + i against the patch, a ballot compaction writes the hits to LDS in
// ascending tile order, and all threads walk that list (the list reads are LDS broadcasts, the loop bounds workgroup-uniform).
// A thread holds its K + 1 canvas values in registers from the first tile to the last and stores them only if a tile covered
// one of its pixels: canvas = fma(w, p, canvas) per class and canvas[K] += w, in ascending tile order whatever the batching.
template <int K, int V, typename Src>
__global__ __launch_bounds__(256) void scene_blend_kernel(Src src, int B, int th, int tw, const int32_t* __restrict__ origins,
                                                          const float* __restrict__ wy, const float* __restrict__ wx,
                                                          float* __restrict__ canvas, int H, int W, int y0, int y1, int x0, int x1,
                                                          int xa, int patches_x) {
  struct alignas(sizeof(float) * V) VecF { float v[V]; };
  constexpr int LPR = PATCH_W / V, PH = 256 / LPR;
  __shared__ int s_tile[256], s_oy[256], s_ox[256], s_count[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int py0 = y0 + (int)(blockIdx.x / patches_x) * PH, px0 = xa + (int)(blockIdx.x % patches_x) * PATCH_W;
  const int py1 = py0 + PH < y1 ? py0 + PH : y1, px1 = px0 + PATCH_W < x1 ? px0 + PATCH_W : x1;
  const int y = py0 + tid / LPR, xb = px0 + (tid % LPR) * V;
  src.prepare();

  bool in[V], any_in = false;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    in[e] = y < y1 && xb + e >= x0 && xb + e < x1;
    any_in |= in[e];
  }
  // V == 4: xb % 4 == 0 and W % 4 == 0, so the four pixels are inside the canvas row as soon as one of them is inside the box
  float acc[K + 1][V];
  float* const mine = canvas + (int64_t)y * W + xb;
  const int64_t plane = (int64_t)H * W;
  if (any_in) {
#pragma unroll
    for (int k = 0; k <= K; ++k) {
      const VecF c = *(const VecF*)(mine + k * plane);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[k][e] = c.v[e];
    }
  }
  bool touched = false;

  for (int base = 0; base < B; base += 256) {
    const int t = base + tid;
    int oy = 0, ox = 0;
    bool hit = false;
    if (t < B) {
      oy = origins[2 * t];
      ox = origins[2 * t + 1];
      hit = oy < py1 && (int64_t)oy + th > py0 && ox < px1 && (int64_t)ox + tw > px0;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_count[wave] = __popcll(m);
    __syncthreads();
    int before = 0, n = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = s_count[w];
      before += w < wave ? c : 0;
      n += c;
    }
    if (hit) {
      const int pos = before + __popcll(m & ((1ull << lane) - 1ull));
      s_tile[pos] = t; s_oy[pos] = oy; s_ox[pos] = ox;
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const int dy = y - s_oy[j], dx0 = xb - s_ox[j];
      if (!any_in || dy < 0 || dy >= th) continue;
      bool cov[V], any = false;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        cov[e] = in[e] && dx0 + e >= 0 && dx0 + e < tw;
        any |= cov[e];
      }
      if (!any) continue;
      float p[V][K];
      src.template load<V>(s_tile[j], dy, dx0, cov, p);
      const float wrow = wy[dy];
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (cov[e]) {
          const float w = wrow * wx[dx0 + e];
#pragma unroll
          for (int k = 0; k < K; ++k) acc[k][e] = fmaf(w, p[e][k], acc[k][e]);
          acc[K][e] += w;
        }
      touched = true;
    }
    __syncthreads();   // the next 256 tiles overwrite the list
  }

  if (touched) {
#pragma unroll
    for (int k = 0; k <= K; ++k) {
      VecF c;
#pragma unroll
      for (int e = 0; e < V; ++e) c.v[e] = acc[k][e];
      *(VecF*)(mine + k * plane) = c;
    }
  }
}

// ------------------------------------------------------------------ finish
// A thread labels V consecutive pixels (V == 4: HW % 4 == 0 and aligned pointers, 16-byte loads of every plane and one 4-byte
// store of the mask).  The class count is a loop bound only: nothing is kept per class.
//
// ND (include/gdlhip_scene_nodata.h): a pixel counts as labelled only where its weight is not 0 and `valid` (if there is one) is
// not 0; every other pixel gets `nodata_label` and probabilities 0.  The quotient and the arg-max are the same expressions.
template <int V, bool ND>
__global__ __launch_bounds__(256) void scene_finish_kernel(const float* __restrict__ canvas, int K, int64_t HW, float threshold,
                                                           uint8_t* __restrict__ mask, float* __restrict__ probs,
                                                           const uint8_t* __restrict__ valid, int nodata_label) {
  struct alignas(sizeof(float) * V) VecF { float v[V]; };
  struct alignas(V) VecB { uint8_t v[V]; };
  const int64_t groups = HW / V;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t i0 = g * V;
    const VecF den = *(const VecF*)(canvas + (int64_t)K * HW + i0);
    [[maybe_unused]] VecB data;      // ND: the plane's bytes, all ones where there is no plane
    if constexpr (ND) {
      if (valid) data = *(const VecB*)(valid + i0);
      else {
#pragma unroll
        for (int e = 0; e < V; ++e) data.v[e] = 1;
      }
    }
    // whether pixel e gets a label and probabilities of its own
    const auto live = [&](int e) {
      if constexpr (ND) return den.v[e] != 0.f && data.v[e] != 0;
      else return den.v[e] != 0.f;
    };
    float best_v[V], first[V];
    int best[V];
    for (int k = 0; k < K; ++k) {
      const VecF c = *(const VecF*)(canvas + (int64_t)k * HW + i0);
      VecF q;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        q.v[e] = canvas_prob(c.v[e], den.v[e], live(e));
        if (k == 0) { best_v[e] = c.v[e]; best[e] = 0; first[e] = q.v[e]; }
        else if (c.v[e] > best_v[e]) { best_v[e] = c.v[e]; best[e] = k; }
      }
      if (probs) *(VecF*)(probs + (int64_t)k * HW + i0) = q;
    }
    VecB o;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int label = K == 1 ? (first[e] > threshold ? 1 : 0) : best[e];
      o.v[e] = live(e) ? (uint8_t)label : (uint8_t)(ND ? nodata_label : 0);
    }
    *(VecB*)(mask + i0) = o;
  }
}

// ------------------------------------------------------------------ nodata (include/gdlhip_scene_nodata.h)
// A thread decides V consecutive pixels (V == 4: W % 4 == 0 and aligned pointers, so every band is one load of 4 samples and the
// plane one 4-byte store).  A sample is nodata when it equals the band's value as a float or, for a NaN value, when it is NaN.
template <typename TI, int V>
__global__ __launch_bounds__(256) void scene_valid_kernel(const TI* __restrict__ raster, int C, int64_t HW, const float* __restrict__ nodata,
                                                          int rule, uint8_t* __restrict__ valid) {
  struct alignas(sizeof(TI) * V) VecT { TI v[V]; };
  struct alignas(V) VecB { uint8_t v[V]; };
  const int64_t groups = HW / V;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t i0 = g * V;
    bool all[V], any[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { all[e] = true; any[e] = false; }
    for (int c = 0; c < C; ++c) {
      const float nd = nodata[c];
      const VecT s = *(const VecT*)(raster + (int64_t)c * HW + i0);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float v = (float)s.v[e];
        const bool is = nd != nd ? v != v : v == nd;
        all[e] = all[e] && is;
        any[e] = any[e] || is;
      }
    }
    VecB o;
#pragma unroll
    for (int e = 0; e < V; ++e) o.v[e] = (rule ? any[e] : all[e]) ? 0 : 1;
    *(VecB*)(valid + i0) = o;
  }
}

// One workgroup per tile: its 256 threads stride over the part of the tile inside the raster (rows y0..y1, columns x0..x1, the
// same in every thread), a wave adds its 64 partial counts by shuffles, the four waves meet in LDS and thread 0 stores the count.
__global__ __launch_bounds__(256) void scene_tile_valid_kernel(const uint8_t* __restrict__ valid, int H, int W,
                                                               const int32_t* __restrict__ origins, int th, int tw,
                                                               int32_t* __restrict__ counts) {
  __shared__ int s_part[4];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int64_t oy = origins[2 * t], ox = origins[2 * t + 1];
  const int64_t y0 = oy < 0 ? 0 : oy, x0 = ox < 0 ? 0 : ox;
  const int64_t y1 = oy + th < H ? oy + th : H, x1 = ox + tw < W ? ox + tw : W;
  int n = 0;
  if (y0 < y1 && x0 < x1) {
    const int cols = (int)(x1 - x0), total = (int)(y1 - y0) * cols;      // at most th * tw, which the entry point holds below 2^31
    for (int i = tid; i < total; i += 256) n += valid[(y0 + i / cols) * W + x0 + i % cols] != 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((tid & 63) == 0) s_part[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) counts[t] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

template <int K, typename Src>
void launch_blend(Src src, int B, int th, int tw, const int32_t* origins, const float* wy, const float* wx, float* canvas, int H, int W,
                  int y0, int y1, int x0, int x1, hipStream_t s) {
  const bool vec = W % 4 == 0 && (uintptr_t)canvas % 16 == 0;
  const int V = vec ? 4 : 1, ph = 256 / (PATCH_W / V);
  const int xa = vec ? x0 & ~3 : x0;
  const int patches_x = (x1 - xa + PATCH_W - 1) / PATCH_W, patches_y = (y1 - y0 + ph - 1) / ph;
  const dim3 grid((unsigned)((int64_t)patches_x * patches_y));
  if (vec) hipLaunchKernelGGL((scene_blend_kernel<K, 4, Src>), grid, dim3(256), 0, s, src, B, th, tw, origins, wy, wx, canvas, H, W, y0, y1, x0, x1, xa, patches_x);
  else hipLaunchKernelGGL((scene_blend_kernel<K, 1, Src>), grid, dim3(256), 0, s, src, B, th, tw, origins, wy, wx, canvas, H, W, y0, y1, x0, x1, xa, patches_x);
}

// the bounding box clipped to the canvas; false = nothing of it is left
bool clip_box(int H, int W, int& y0, int& y1, int& x0, int& x1) {
  y0 = y0 < 0 ? 0 : y0; x0 = x0 < 0 ? 0 : x0;
  y1 = y1 > H ? H : y1; x1 = x1 > W ? W : x1;
  return y0 < y1 && x0 < x1;
}

// gdl_scene_cut, gdl_scene_cut_d4 (d4: xforms != nullptr) and gdl_scene_cut_valid (masked: valid != nullptr): one body, `fn` is
// the entry point's name in the messages
int scene_cut(const char* fn, const void* raster, int kind, int C, int H, int W, const uint8_t* valid, bool masked, const int32_t* origins,
              const int32_t* xforms, bool d4, int B, int th, int tw, int fill, float* tiles, int image_min, int image_max,
              double norm_min, double norm_max, const float* mean, const float* stdv, gdl_stream_t stream) {
  GDL_CHECK_ARG(raster && origins && tiles && mean && stdv && (xforms || !d4) && (valid || !masked), "%s: null pointer", fn);
  GDL_CHECK_ARG(kind >= GDL_RAW_U8 && kind <= GDL_RAW_F32, "%s: bad sample kind %d", fn, kind);
  GDL_CHECK_ARG(C > 0 && H > 0 && W > 0 && B > 0 && th > 0 && tw > 0, "%s: bad sizes", fn);
  GDL_CHECK_ARG(image_max != image_min, "%s: image_max == image_min (%d): the range is empty", fn, image_min);
  const RangeScalars r = range_scalars(image_min, image_max, norm_min, norm_max);
  const bool vec = tw % 4 == 0 && (uintptr_t)tiles % 16 == 0;
  const int64_t groups = (int64_t)B * C * th * (tw / (vec ? 4 : 1));
  hipStream_t s = (hipStream_t)stream;
#define CUT_V(T, V, D4, M)                                                                                                               \
  hipLaunchKernelGGL((scene_cut_kernel<T, V, D4, M>), dim3(grid_for(groups)), dim3(256), 0, s, (const T*)raster, C, H, W, origins, xforms, \
                     th, tw, (float)fill, tiles, groups, r.imin, r.span, r.d, r.nmin, mean, stdv, valid)
#define CUT_D(T, D4)                                                                     \
  if (masked) { if (vec) CUT_V(T, 4, D4, true); else CUT_V(T, 1, D4, true); }            \
  else { if (vec) CUT_V(T, 4, D4, false); else CUT_V(T, 1, D4, false); }
#define CUT(T) \
  if (d4) { CUT_D(T, true) } else { CUT_D(T, false) }
  if (kind == GDL_RAW_U8) { CUT(uint8_t) }
  else if (kind == GDL_RAW_U16) { CUT(uint16_t) }
  else if (kind == GDL_RAW_I16) { CUT(int16_t) }
  else { CUT(float) }
#undef CUT
#undef CUT_D
#undef CUT_V
  GDL_CHECK_LAUNCH(fn);
  return GDL_OK;
}

}  // namespace

extern "C" int gdl_scene_cut(const void* raster, int kind, int C, int H, int W, const int32_t* origins, int B, int th, int tw, int fill,
                             float* tiles, int image_min, int image_max, double norm_min, double norm_max, const float* mean,
                             const float* stdv, gdl_stream_t stream) {
  return scene_cut("gdl_scene_cut", raster, kind, C, H, W, nullptr, false, origins, nullptr, false, B, th, tw, fill, tiles, image_min, image_max, norm_min,
                   norm_max, mean, stdv, stream);
}

extern "C" int gdl_scene_cut_d4(const void* raster, int kind, int C, int H, int W, const int32_t* origins, const int32_t* xforms, int B,
                                int th, int tw, int fill, float* tiles, int image_min, int image_max, double norm_min, double norm_max,
                                const float* mean, const float* stdv, gdl_stream_t stream) {
  return scene_cut("gdl_scene_cut_d4", raster, kind, C, H, W, nullptr, false, origins, xforms, true, B, th, tw, fill, tiles, image_min, image_max,
                   norm_min, norm_max, mean, stdv, stream);
}

extern "C" int gdl_scene_blend(const float* probs, int B, int K, int th, int tw, const int32_t* origins, const float* wy,
                               const float* wx, float* canvas, int H, int W, int y0, int y1, int x0, int x1, gdl_stream_t stream) {
  GDL_CHECK_ARG(probs && origins && wy && wx && canvas, "gdl_scene_blend: null pointer");
  GDL_CHECK_ARG(B > 0 && th > 0 && tw > 0 && H > 0 && W > 0, "gdl_scene_blend: bad sizes");
  GDL_CHECK_ARG(K >= 1 && K <= 16, "gdl_scene_blend: 1..16 classes, got %d", K);
  if (!clip_box(H, W, y0, y1, x0, x1)) return GDL_OK;
  const bool vec = tw % 4 == 0 && (uintptr_t)probs % 16 == 0;
  K_SWITCH(K, launch_blend<KK>(ProbsSource<KK>{probs, th, tw, vec}, B, th, tw, origins, wy, wx, canvas, H, W, y0, y1, x0, x1, (hipStream_t)stream));
  GDL_CHECK_LAUNCH("gdl_scene_blend");
  return GDL_OK;
}

extern "C" int gdl_scene_blend_d4(const float* probs, int B, int K, int th, int tw, const int32_t* origins, const int32_t* xforms,
                                  const float* wy, const float* wx, float* canvas, int H, int W, int y0, int y1, int x0, int x1,
                                  gdl_stream_t stream) {
  GDL_CHECK_ARG(probs && origins && xforms && wy && wx && canvas, "gdl_scene_blend_d4: null pointer");
  GDL_CHECK_ARG(B > 0 && th > 0 && tw > 0 && H > 0 && W > 0, "gdl_scene_blend_d4: bad sizes");
  GDL_CHECK_ARG(K >= 1 && K <= 16, "gdl_scene_blend_d4: 1..16 classes, got %d", K);
  if (!clip_box(H, W, y0, y1, x0, x1)) return GDL_OK;
  const bool vec = tw % 4 == 0 && (uintptr_t)probs % 16 == 0;
  K_SWITCH(K, launch_blend<KK>(ProbsSourceD4<KK>{probs, xforms, th, tw, vec}, B, th, tw, origins, wy, wx, canvas, H, W, y0, y1, x0, x1, (hipStream_t)stream));
  GDL_CHECK_LAUNCH("gdl_scene_blend_d4");
  return GDL_OK;
}

extern "C" int gdl_scene_blend_lowres(const float* low, int B, int hi, int wi, int K, int th, int tw, const int32_t* origins,
                                      const float* wy, const float* wx, float* canvas, int H, int W, int y0, int y1, int x0, int x1,
                                      gdl_stream_t stream) {
  GDL_CHECK_ARG(low && origins && wy && wx && canvas, "gdl_scene_blend_lowres: null pointer");
  GDL_CHECK_ARG(B > 0 && hi > 0 && wi > 0 && th > 0 && tw > 0 && H > 0 && W > 0, "gdl_scene_blend_lowres: bad sizes");
  GDL_CHECK_ARG(K >= 1 && K <= 16, "gdl_scene_blend_lowres: 1..16 classes, got %d (more: gdl_class_probs + gdl_scene_blend)", K);
  if (!clip_box(H, W, y0, y1, x0, x1)) return GDL_OK;
  K_SWITCH(K, launch_blend<KK>(LowresSource<KK>{low, hi, wi, th, tw, 0.f, 0.f}, B, th, tw, origins, wy, wx, canvas, H, W, y0, y1, x0, x1, (hipStream_t)stream));
  GDL_CHECK_LAUNCH("gdl_scene_blend_lowres");
  return GDL_OK;
}

extern "C" int gdl_scene_blend_lowres_d4(const float* low, int B, int hi, int wi, int K, int th, int tw, const int32_t* origins,
                                         const int32_t* xforms, const float* wy, const float* wx, float* canvas, int H, int W, int y0,
                                         int y1, int x0, int x1, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && origins && xforms && wy && wx && canvas, "gdl_scene_blend_lowres_d4: null pointer");
  GDL_CHECK_ARG(B > 0 && hi > 0 && wi > 0 && th > 0 && tw > 0 && H > 0 && W > 0, "gdl_scene_blend_lowres_d4: bad sizes");
  GDL_CHECK_ARG(K >= 1 && K <= 16, "gdl_scene_blend_lowres_d4: 1..16 classes, got %d (more: gdl_class_probs + gdl_scene_blend_d4)", K);
  if (!clip_box(H, W, y0, y1, x0, x1)) return GDL_OK;
  K_SWITCH(K, launch_blend<KK>(LowresSourceD4<KK>{low, xforms, hi, wi, th, tw, 0.f, 0.f}, B, th, tw, origins, wy, wx, canvas, H, W, y0, y1, x0, x1, (hipStream_t)stream));
  GDL_CHECK_LAUNCH("gdl_scene_blend_lowres_d4");
  return GDL_OK;
}

extern "C" int gdl_scene_finish(const float* canvas, int K, int64_t HW, float threshold, uint8_t* mask, float* probs,
                                gdl_stream_t stream) {
  GDL_CHECK_ARG(canvas && mask, "gdl_scene_finish: null pointer");
  GDL_CHECK_ARG(K >= 1 && K <= 255 && HW > 0, "gdl_scene_finish: bad sizes (1..255 classes, got %d)", K);
  const bool vec = HW % 4 == 0 && (uintptr_t)canvas % 16 == 0 && (uintptr_t)probs % 16 == 0 && (uintptr_t)mask % 4 == 0;
  hipStream_t s = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL((scene_finish_kernel<4, false>), dim3(grid_for(HW / 4)), dim3(256), 0, s, canvas, K, HW, threshold, mask, probs, nullptr, 0);
  else hipLaunchKernelGGL((scene_finish_kernel<1, false>), dim3(grid_for(HW)), dim3(256), 0, s, canvas, K, HW, threshold, mask, probs, nullptr, 0);
  GDL_CHECK_LAUNCH("gdl_scene_finish");
  return GDL_OK;
}

// ------------------------------------------------------------------ nodata (include/gdlhip_scene_nodata.h)
extern "C" int gdl_scene_valid(const void* raster, int kind, int C, int H, int W, const float* nodata, int rule, uint8_t* valid,
                               gdl_stream_t stream) {
  GDL_CHECK_ARG(raster && nodata && valid, "gdl_scene_valid: null pointer");
  GDL_CHECK_ARG(kind >= GDL_RAW_U8 && kind <= GDL_RAW_F32, "gdl_scene_valid: bad sample kind %d", kind);
  GDL_CHECK_ARG(C > 0 && H > 0 && W > 0, "gdl_scene_valid: bad sizes");
  GDL_CHECK_ARG(rule == 0 || rule == 1, "gdl_scene_valid: rule %d is neither 0 (all bands) nor 1 (any band)", rule);
  const int64_t HW = (int64_t)H * W;
  const size_t esz = kind == GDL_RAW_U8 ? 1 : kind == GDL_RAW_F32 ? 4 : 2;
  const bool vec = W % 4 == 0 && (uintptr_t)raster % (4 * esz) == 0 && (uintptr_t)valid % 4 == 0;
  hipStream_t s = (hipStream_t)stream;
#define VALID(T)                                                                                                                          \
  if (vec) hipLaunchKernelGGL((scene_valid_kernel<T, 4>), dim3(grid_for(HW / 4)), dim3(256), 0, s, (const T*)raster, C, HW, nodata, rule, valid); \
  else hipLaunchKernelGGL((scene_valid_kernel<T, 1>), dim3(grid_for(HW)), dim3(256), 0, s, (const T*)raster, C, HW, nodata, rule, valid);
  if (kind == GDL_RAW_U8) { VALID(uint8_t) }
  else if (kind == GDL_RAW_U16) { VALID(uint16_t) }
  else if (kind == GDL_RAW_I16) { VALID(int16_t) }
  else { VALID(float) }
#undef VALID
  GDL_CHECK_LAUNCH("gdl_scene_valid");
  return GDL_OK;
}

extern "C" int gdl_scene_tile_valid(const uint8_t* valid, int H, int W, const int32_t* origins, int T, int th, int tw, int32_t* counts,
                                    gdl_stream_t stream) {
  GDL_CHECK_ARG(valid && origins && counts, "gdl_scene_tile_valid: null pointer");
  GDL_CHECK_ARG(H > 0 && W > 0 && T > 0 && th > 0 && tw > 0, "gdl_scene_tile_valid: bad sizes");
  GDL_CHECK_ARG((int64_t)th * tw <= INT32_MAX, "gdl_scene_tile_valid: a tile of %d x %d pixels does not count in an int32", th, tw);
  hipLaunchKernelGGL(scene_tile_valid_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, valid, H, W, origins, th, tw, counts);
  GDL_CHECK_LAUNCH("gdl_scene_tile_valid");
  return GDL_OK;
}

extern "C" int gdl_scene_cut_valid(const void* raster, int kind, int C, int H, int W, const uint8_t* valid, const int32_t* origins,
                                   const int32_t* xforms, int B, int th, int tw, int fill, float* tiles, int image_min, int image_max,
                                   double norm_min, double norm_max, const float* mean, const float* stdv, gdl_stream_t stream) {
  return scene_cut("gdl_scene_cut_valid", raster, kind, C, H, W, valid, true, origins, xforms, xforms != nullptr, B, th, tw, fill, tiles,
                   image_min, image_max, norm_min, norm_max, mean, stdv, stream);
}

extern "C" int gdl_scene_finish_valid(const float* canvas, int K, int64_t HW, float threshold, const uint8_t* valid, int nodata_label,
                                      uint8_t* mask, float* probs, gdl_stream_t stream) {
  GDL_CHECK_ARG(canvas && mask, "gdl_scene_finish_valid: null pointer");
  GDL_CHECK_ARG(K >= 1 && K <= 255 && HW > 0, "gdl_scene_finish_valid: bad sizes (1..255 classes, got %d)", K);
  GDL_CHECK_ARG(nodata_label >= 0 && nodata_label <= 255, "gdl_scene_finish_valid: nodata_label %d is not in 0..255", nodata_label);
  const bool vec = HW % 4 == 0 && (uintptr_t)canvas % 16 == 0 && (uintptr_t)probs % 16 == 0 && (uintptr_t)mask % 4 == 0 && (uintptr_t)valid % 4 == 0;
  hipStream_t s = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL((scene_finish_kernel<4, true>), dim3(grid_for(HW / 4)), dim3(256), 0, s, canvas, K, HW, threshold, mask, probs, valid, nodata_label);
  else hipLaunchKernelGGL((scene_finish_kernel<1, true>), dim3(grid_for(HW)), dim3(256), 0, s, canvas, K, HW, threshold, mask, probs, valid, nodata_label);
  GDL_CHECK_LAUNCH("gdl_scene_finish_valid");
  return GDL_OK;
}
