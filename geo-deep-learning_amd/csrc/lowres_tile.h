// What the per-pixel losses share (loss_ce.hip: soft cross-entropy; loss_focal.hip: focal; loss_bce.hip: soft BCE): the f64 partial-sum helpers, and the
// tile form of the low-resolution backward.  A per-pixel loss's gradient needs no global sum, so a workgroup that owns a
// CT_H x CT_W tile of full-resolution pixels can
//   1. write dL/dlogit of its pixels (unscaled) to LDS            -- the loss's own kernel, the only part that differs;
//   2. apply the transposed bilinear resize over rows, 3. over columns -> the tile's partial patch (lowres_tile_patch);
// lowres_reduce_kernel then adds, per low-resolution logit vector, the patches of the (at most four) tiles that touch it in a
// fixed order and applies the scalar factors.  No float atomics; K <= 8 (LDS).
#pragma once
#include "gdl_common.h"
#include "bilinear_index.h"

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// 256 threads: the workgroup's sum of `acc` (f64, fixed order) -> ws[blockIdx.x]
__device__ __forceinline__ void block256_store_sum(double acc, double* __restrict__ ws) {
  __shared__ double red[4];
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ws[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

constexpr int LOWRES_MAX_FACTOR = 64;   // bounds the gather kernels' window: (2 * factor + 4)^2 evaluations per logit vector

constexpr int CT_H = 32, CT_W = 64, CT_MAXN = 36;
constexpr int CT_T = 1024;

struct LowresTile {
  const float* low; const int64_t* target; const float* upstream; double* tile_loss; float* patches; float* dlow;
  const float* norm;      // device scalar multiplied into the reduce's factor (the focal loss's 1 / valid count); null: 1
  int B, Hi, Wi, Ho, Wo, tiles_y, tiles_x, ny_max, nx_max;
  float scale;
};

// low-resolution rows / columns one tile side can touch: CT * ratio + 2 (an upper bound for ratios <= 1); false: the shape
// does not take the tile form
inline bool lowres_tile_dims(int K, int Hi, int Wi, int Ho, int Wo, int& ny_max, int& nx_max) {
  ny_max = (int)((int64_t)CT_H * Hi / Ho) + 3;
  nx_max = (int)((int64_t)CT_W * Wi / Wo) + 3;
  return K <= 8 && ny_max <= CT_MAXN && nx_max <= CT_MAXN + CT_MAXN;
}
// one class (the binary losses): a 1:1 "resize" shares no pixel between low-resolution logits -- the gather kernel evaluates every
// pixel exactly once there, so it is the only form
inline bool binary_tile_dims(int Hi, int Wi, int Ho, int Wo, int& ny_max, int& nx_max) {
  return lowres_tile_dims(1, Hi, Wi, Ho, Wo, ny_max, nx_max) && !(Ho == Hi && Wo == Wi);
}
inline int64_t lowres_tiles(int B, int Ho, int Wo) { return (int64_t)B * ((Ho + CT_H - 1) / CT_H) * ((Wo + CT_W - 1) / CT_W); }
inline size_t lowres_tile_lds(int K, int ny, int nx) {
  return ((size_t)K * CT_H * CT_W + (size_t)K * ny * (CT_W + 1) + (size_t)ny * CT_H + (size_t)nx * CT_W) * sizeof(float);
}
inline void lowres_tile_shape(LowresTile& a, int B, int Hi, int Wi, int Ho, int Wo, int ny, int nx) {
  a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo;
  a.tiles_y = (Ho + CT_H - 1) / CT_H; a.tiles_x = (Wo + CT_W - 1) / CT_W; a.ny_max = ny; a.nx_max = nx;
}

// the tile of workgroup blockIdx.x
struct TileAt {
  int b, oy0, ox0, rows, cols;
  float ry, rx;
};
__device__ __forceinline__ TileAt lowres_tile_at(const LowresTile& a) {
  TileAt t;
  const int tx = blockIdx.x % a.tiles_x, ty = (blockIdx.x / a.tiles_x) % a.tiles_y;
  t.b = blockIdx.x / (a.tiles_x * a.tiles_y);
  t.oy0 = ty * CT_H; t.ox0 = tx * CT_W;
  t.rows = a.Ho - t.oy0 < CT_H ? a.Ho - t.oy0 : CT_H; t.cols = a.Wo - t.ox0 < CT_W ? a.Wo - t.ox0 : CT_W;
  t.ry = (float)a.Hi / (float)a.Ho; t.rx = (float)a.Wi / (float)a.Wo;
  return t;
}

// Steps 2 and 3 for the tile whose unscaled dL/dlogit sits in csm as dl[K][CT_H][CT_W] (zeros outside the image and at
// ignored pixels).  Called by all CT_T threads after they wrote dl and BEFORE any barrier: the first barrier is in here, after
// the two 1-D weight tables; `between` runs on every thread right after it (the CE kernel stores its loss partial there).
template <int K, typename F>
__device__ __forceinline__ void lowres_tile_patch(const LowresTile& a, const TileAt& t, float* csm, F between) {
  float* dl = csm;                                   // [K][CT_H][CT_W]
  float* tmp = csm + K * CT_H * CT_W;                // [K][ny_max][CT_W + 1]
  float* wyt = tmp + K * a.ny_max * (CT_W + 1);      // [ny_max][CT_H]  weight of tile row r for low-resolution row iy_lo + j
  float* wxt = wyt + a.ny_max * CT_H;                // [nx_max][CT_W]  the same for columns
  const int tid = threadIdx.x;
  const int oy0 = t.oy0, ox0 = t.ox0, rows = t.rows, cols = t.cols;
  const float ry = t.ry, rx = t.rx;
  // the low-resolution rows iy_lo .. iy_hi / columns ix_lo .. ix_hi this tile touches, and the two 1-D weight tables
  int iy_lo, iy_hi, ix_lo, ix_hi;
  touched_range(ry, oy0, oy0 + rows - 1, a.Hi, iy_lo, iy_hi);
  touched_range(rx, ox0, ox0 + cols - 1, a.Wi, ix_lo, ix_hi);
  const int ny = iy_hi - iy_lo + 1, nx = ix_hi - ix_lo + 1;
  for (int i = tid; i < ny * CT_H; i += CT_T) {
    const int j = i / CT_H, r = i - j * CT_H;
    float wv = 0.f;
    if (r < rows) {
      int y0, y1; float ly;
      src_index2(ry, oy0 + r, a.Hi, y0, y1, ly);
      wv = (y0 == iy_lo + j ? 1.f - ly : 0.f) + (y1 == iy_lo + j ? ly : 0.f);
    }
    wyt[i] = wv;
  }
  for (int i = tid; i < nx * CT_W; i += CT_T) {
    const int q = i / CT_W, c = i - q * CT_W;
    float wv = 0.f;
    if (c < cols) {
      int x0, x1; float lx;
      src_index2(rx, ox0 + c, a.Wi, x0, x1, lx);
      wv = (x0 == ix_lo + q ? 1.f - lx : 0.f) + (x1 == ix_lo + q ? lx : 0.f);
    }
    wxt[i] = wv;
  }
  __syncthreads();
  between();
  // ---- 2. rows
  for (int i = tid; i < ny * CT_W; i += CT_T) {
    const int j = i / CT_W, c = i - j * CT_W;
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    int r_lo, r_hi;      // only the tile rows that can interpolate from low-resolution row iy_lo + j
    cand_range(iy_lo + j, ry, a.Ho, r_lo, r_hi);
    r_lo = r_lo - oy0 < 0 ? 0 : r_lo - oy0;
    r_hi = r_hi - oy0 > rows - 1 ? rows - 1 : r_hi - oy0;
    for (int r = r_lo; r <= r_hi; ++r) {
      const float wy = wyt[j * CT_H + r];
      if (wy != 0.f) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += wy * dl[(k * CT_H + r) * CT_W + c];
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) tmp[(k * a.ny_max + j) * (CT_W + 1) + c] = acc[k];
  }
  __syncthreads();
  // ---- 3. columns -> the tile's partial patch [ny_max][nx_max][K] (entries beyond ny / nx are never read)
  float* patch = a.patches + (int64_t)blockIdx.x * a.ny_max * a.nx_max * K;
  for (int i = tid; i < ny * nx; i += CT_T) {
    const int j = i / nx, q = i - j * nx;
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    int c_lo, c_hi;
    cand_range(ix_lo + q, rx, a.Wo, c_lo, c_hi);
    c_lo = c_lo - ox0 < 0 ? 0 : c_lo - ox0;
    c_hi = c_hi - ox0 > cols - 1 ? cols - 1 : c_hi - ox0;
    for (int c = c_lo; c <= c_hi; ++c) {
      const float wx = wxt[q * CT_W + c];
      if (wx != 0.f) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += wx * tmp[(k * a.ny_max + j) * (CT_W + 1) + c];
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) patch[(j * a.nx_max + q) * K + k] = acc[k];
  }
}

template <int K>
__global__ __launch_bounds__(256) void lowres_reduce_kernel(const LowresTile a) {
  float cf = (a.upstream ? a.upstream[0] : 1.f) * a.scale;
  if (a.norm) cf *= a.norm[0];
  const int64_t total = (int64_t)a.B * a.Hi * a.Wi;
  const float ry = (float)a.Hi / (float)a.Ho, rx = (float)a.Wi / (float)a.Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i % a.Wi);
    const int64_t r = i / a.Wi;
    const int iy = (int)(r % a.Hi), b = (int)(r / a.Hi);
    int ylo, yhi, xlo, xhi;
    cand_range(iy, ry, a.Ho, ylo, yhi);              // full-resolution rows / columns that can interpolate from (iy, ix)
    cand_range(ix, rx, a.Wo, xlo, xhi);
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    for (int ty = ylo / CT_H; ty <= yhi / CT_H; ++ty) {
      const int oy0 = ty * CT_H, rows = a.Ho - oy0 < CT_H ? a.Ho - oy0 : CT_H;
      int iy_lo, iy_hi;
      touched_range(ry, oy0, oy0 + rows - 1, a.Hi, iy_lo, iy_hi);
      if (iy < iy_lo || iy > iy_hi) continue;
      for (int tx = xlo / CT_W; tx <= xhi / CT_W; ++tx) {
        const int ox0 = tx * CT_W, cols = a.Wo - ox0 < CT_W ? a.Wo - ox0 : CT_W;
        int ix_lo, ix_hi;
        touched_range(rx, ox0, ox0 + cols - 1, a.Wi, ix_lo, ix_hi);
        if (ix < ix_lo || ix > ix_hi) continue;
        const float* patch = a.patches + ((int64_t)(b * a.tiles_y + ty) * a.tiles_x + tx) * a.ny_max * a.nx_max * K;
        const float* src = patch + ((iy - iy_lo) * a.nx_max + (ix - ix_lo)) * K;
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += src[k];
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) a.dlow[i * K + k] = cf * acc[k];
  }
}

inline int lowres_launch_reduce(const LowresTile& a, int K, hipStream_t st) {
  const int64_t total = (int64_t)a.B * a.Hi * a.Wi;
  K_SWITCH(K, if (KK <= 8) hipLaunchKernelGGL((lowres_reduce_kernel<(KK <= 8 ? KK : 8)>), dim3(grid_for(total)), dim3(256), 0, st, a));
  return GDL_OK;
}

}  // namespace
