// What the per-pixel and one-class losses share (loss_ce.hip: soft cross-entropy; loss_xent.hip: weighted cross-entropy;
// loss_focal.hip: focal, multiclass and binary; loss_bce.hip: soft BCE; loss_dice.hip: the binary Dice family): the f64
// partial-sum helpers and the three low-resolution kernel skeletons, each parametrised by the class count K and the loss's per-pixel policy `Pix` -- the only part that differs:
//   lowres_partial_kernel     forward: per-workgroup f64 partial sums of the loss over the on-the-fly bilinear logits
//   lowres_gather_bwd_kernel  backward, gather form: one thread per low-resolution logit vector (K <= 16)
//   lowres_tile_front_kernel  backward, tile form (K <= 8, LDS).  A per-pixel gradient needs no global sum, so a workgroup that
//                             owns a CT_H x CT_W tile of full-resolution pixels
//     1. writes dL/dlogit of its pixels (unscaled) to LDS                                      -- Pix::grad;
//     2. applies the transposed bilinear resize over rows, 3. over columns -> the tile's partial patch (lowres_tile_patch);
//   lowres_reduce_kernel then adds, per low-resolution logit vector, the patches of the (at most four) tiles that touch it in
//   a fixed order and applies the scalar factors.
// No float atomics.  lowres_bwd() is the one host-side choice between the two backward forms.
//
// A policy is a trivially copyable struct built once per thread as Pix(opt, K); it holds what the loss hoists out of the pixel loop:
//   Opt, Target        the loss's option struct (a kernel argument) and the target's element type
//   ONE_CLASS          K is always 1 (the one-class losses): only that instantiation exists, and a 1:1 resize has no tile form
//   COUNTS             the forward also stores, at ws[gridDim.x ..), the per-workgroup sum of count(t) over the valid pixels: the
//                      divisor of a mean the loss forms on the device (mean_final.h)
//   count(t)           (COUNTS only) what a valid pixel adds to that divisor: 1 (focal), the target class's weight (cross-entropy)
//   valid(t)           false: the pixel adds nothing (tested BEFORE its logits are evaluated)
//   grad(x, t, g)      the K bilinear logits x (may be overwritten) and target t -> the unscaled dL/dlogit in g[K]
//   loss(x, t)         the pixel's loss (forward)
//   grad_loss(x, t, g) both from one evaluation; only where the tile kernel is instantiated with LOSS (soft CE's fused form)
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
  const float* low;
  const void* target;     // [B, Ho, Wo] of the policy's Target
  const float* upstream; double* tile_loss; float* patches; float* dlow;
  const float* norm;      // device scalar multiplied into the final factor (the divisor mean_final.h left); null: 1
  int B, Hi, Wi, Ho, Wo, tiles_y, tiles_x, ny_max, nx_max;
  float scale;
};
// the argument of both backward forms: the tile kernel, the reduce and the gather kernel read the same fields
template <typename Opt>
struct LowresArgs : LowresTile {
  Opt o;
};
// upstream * scale * norm: the one factor applied at the end of either form
__device__ __forceinline__ float lowres_factor(const LowresTile& a) {
  float cf = (a.upstream ? a.upstream[0] : 1.f) * a.scale;
  if (a.norm) cf *= a.norm[0];
  return cf;
}

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
// the two 1-D weight tables; `between` runs on every thread right after it (the tile's loss partial is stored there).
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
  const float cf = lowres_factor(a);
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

// ------------------------------------------------------------------ the three skeletons
// forward: ws[0 .. gridDim.x) = f64 partial sums of the loss over the valid pixels; with Pix::COUNTS, ws[gridDim.x .. 2 gridDim.x) =
// the sums of Pix::count() over them (a count of pixels is exact in f64)
template <int K, typename Pix>
__global__ __launch_bounds__(256) void lowres_partial_kernel(const float* __restrict__ low, const typename Pix::Target* __restrict__ target,
                                                             int B, int Hi, int Wi, int Ho, int Wo, double* __restrict__ ws,
                                                             const typename Pix::Opt o) {
  const Pix pix(o, K);
  const int64_t total = (int64_t)B * Ho * Wo;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  double acc = 0.0, cnt = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const typename Pix::Target t = target[i];
    if (!pix.valid(t)) continue;
    const int ox = (int)(i % Wo);
    const int64_t r = i / Wo;
    const int oy = (int)(r % Ho), b = (int)(r / Ho);
    int y0, y1, x0, x1; float ly, lx;
    src_index2(ry, oy, Hi, y0, y1, ly);
    src_index2(rx, ox, Wi, x0, x1, lx);
    float x[K];
    bilinear_logits<K>(low, b, Hi, Wi, y0, y1, x0, x1, ly, lx, x);
    acc += (double)pix.loss(x, t);
    if constexpr (Pix::COUNTS) cnt += (double)pix.count(t);
  }
  block256_store_sum(acc, ws);
  if constexpr (Pix::COUNTS) {
    __syncthreads();      // block256_store_sum's LDS slots are reused
    block256_store_sum(cnt, ws + gridDim.x);
  }
}

// gather form: one thread per LOW-resolution logit vector sums wy * wx * dL/dlogit over the full-resolution pixels that interpolate
// from it, rows then columns in ascending order.  Every class count up to 16; each full-resolution pixel is evaluated once per
// low-resolution neighbour (up to four times).
template <int K, typename Pix>
__global__ __launch_bounds__(256) void lowres_gather_bwd_kernel(const LowresArgs<typename Pix::Opt> a) {
  const typename Pix::Target* __restrict__ target = (const typename Pix::Target*)a.target;
  const Pix pix(a.o, K);
  const float cf = lowres_factor(a);
  const int64_t total = (int64_t)a.B * a.Hi * a.Wi;
  const float ry = (float)a.Hi / (float)a.Ho, rx = (float)a.Wi / (float)a.Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i % a.Wi);
    const int64_t r = i / a.Wi;
    const int iy = (int)(r % a.Hi), b = (int)(r / a.Hi);
    int ylo, yhi, xlo, xhi;
    cand_range(iy, ry, a.Ho, ylo, yhi);
    cand_range(ix, rx, a.Wo, xlo, xhi);
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
      int y0, y1; float ly;
      src_index2(ry, oy, a.Hi, y0, y1, ly);
      const float wy = (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
      if (wy == 0.f) continue;
      const int64_t trow = ((int64_t)b * a.Ho + oy) * a.Wo;
#pragma unroll 1
      for (int ox = xlo; ox <= xhi; ++ox) {
        int x0, x1; float lx;
        src_index2(rx, ox, a.Wi, x0, x1, lx);
        const float w = wy * ((x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f));
        if (w == 0.f) continue;
        const typename Pix::Target t = target[trow + ox];
        if (!pix.valid(t)) continue;      // an ignored pixel adds nothing
        float x[K], g[K];
        bilinear_logits<K>(a.low, b, a.Hi, a.Wi, y0, y1, x0, x1, ly, lx, x);
        pix.grad(x, t, g);
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += w * g[k];
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) a.dlow[i * K + k] = cf * acc[k];
  }
}

// tile form, step 1: dL/dlogit of the tile's pixels (unscaled; zeros outside the image and at ignored pixels) -> LDS; with LOSS also
// the tile's loss sum (f64) -> tile_loss[tile]; then the shared transposed resize into the tile's partial patch.  Every
// full-resolution pixel is evaluated once; lowres_reduce_kernel applies lowres_factor().  K <= 8.
template <int K, typename Pix, bool LOSS>
__global__ __launch_bounds__(CT_T) void lowres_tile_front_kernel(const LowresArgs<typename Pix::Opt> a) {
  extern __shared__ __attribute__((aligned(16))) float csm[];
  __shared__ double lred[CT_T / 64];
  float* dl = csm;                                   // [K][CT_H][CT_W]
  const typename Pix::Target* __restrict__ target = (const typename Pix::Target*)a.target;
  const int tid = threadIdx.x;
  const TileAt at = lowres_tile_at(a);
  const Pix pix(a.o, K);
  double lacc = 0.0;
  for (int i = tid; i < CT_H * CT_W; i += CT_T) {
    const int r = i / CT_W, c = i - r * CT_W;
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.f;
    if (r < at.rows && c < at.cols) {
      const int oy = at.oy0 + r, ox = at.ox0 + c;
      const typename Pix::Target t = target[((int64_t)at.b * a.Ho + oy) * a.Wo + ox];
      if (pix.valid(t)) {
        int y0, y1, x0, x1; float ly, lx;
        src_index2(at.ry, oy, a.Hi, y0, y1, ly);
        src_index2(at.rx, ox, a.Wi, x0, x1, lx);
        float x[K];
        bilinear_logits<K>(a.low, at.b, a.Hi, a.Wi, y0, y1, x0, x1, ly, lx, x);
        if constexpr (LOSS) lacc += (double)pix.grad_loss(x, t, v);
        else pix.grad(x, t, v);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) dl[(k * CT_H + r) * CT_W + c] = v[k];
  }
  if constexpr (LOSS) {
    lacc = wave_sum_f64(lacc);
    if ((tid & 63) == 0) lred[tid >> 6] = lacc;
  }
  lowres_tile_patch<K>(a, at, csm, [&] {
    if constexpr (LOSS) {
      if (tid == 0) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < CT_T / 64; ++w) s += lred[w];
        a.tile_loss[blockIdx.x] = s;
      }
    }
  });
}

// ------------------------------------------------------------------ host side
#define LOWRES_SHAPE(who, K)                                                                                                      \
  GDL_CHECK_ARG(B > 0 && Hi > 0 && Wi > 0 && Ho >= Hi && Wo >= Wi, "%s: bad sizes (an upsample is expected)", who);               \
  GDL_CHECK_ARG((Ho + Hi - 1) / Hi <= LOWRES_MAX_FACTOR && (Wo + Wi - 1) / Wi <= LOWRES_MAX_FACTOR,                               \
                "%s: upsampling factors above 64 are not supported", who);                                                        \
  GDL_CHECK_ARG(K >= 1 && K <= 16, "%s: K=%d classes unsupported (1..16)", who, K)

// `__VA_ARGS__` with KK = the class count as a compile-time constant: 1 for a one-class policy, K_SWITCH otherwise
#define LOWRES_K_SWITCH(Pix, K, ...)                                   \
  if constexpr (Pix::ONE_CLASS) { constexpr int KK = 1; __VA_ARGS__; } \
  else { K_SWITCH(K, __VA_ARGS__); }

// workgroups of the forward (1024 pixels each, up to 2048: the scattered loads of the on-the-fly logit are latency bound)
inline int lowres_fwd_blocks(int64_t total) {
  int64_t g = (total + 1023) / 1024;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

// launches the forward's partial sums into ws; nblk = the number of partials (lowres_fwd_blocks)
template <typename Pix>
int lowres_launch_partial(const float* low, const void* target, int B, int K, int Hi, int Wi, int Ho, int Wo, double* ws,
                          const typename Pix::Opt& o, int& nblk, hipStream_t st) {
  nblk = lowres_fwd_blocks((int64_t)B * Ho * Wo);
  LOWRES_K_SWITCH(Pix, K, hipLaunchKernelGGL((lowres_partial_kernel<KK, Pix>), dim3(nblk), dim3(256), 0, st, low,
                                             (const typename Pix::Target*)target, B, Hi, Wi, Ho, Wo, ws, o));
  return GDL_OK;
}

template <typename Opt>
LowresArgs<Opt> lowres_args(const float* low, const void* target, int B, int Hi, int Wi, int Ho, int Wo, const float* upstream,
                            float scale, const float* norm, float* dlow, const Opt& o) {
  LowresArgs<Opt> a{};
  a.low = low; a.target = target; a.upstream = upstream; a.scale = scale; a.norm = norm; a.dlow = dlow; a.o = o;
  a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo;
  return a;
}

// bytes of patches the tile form needs; 0: the shape takes the gather kernel only.  one_class: the rule of binary_tile_dims.
inline int64_t lowres_bwd_need(int K, bool one_class, int B, int Hi, int Wi, int Ho, int Wo) {
  int ny, nx;
  if (B <= 0 || K < 1 || Hi <= 0 || Wi <= 0 || Ho < Hi || Wo < Wi) return 0;
  if (!(one_class ? binary_tile_dims(Hi, Wi, Ho, Wo, ny, nx) : lowres_tile_dims(K, Hi, Wi, Ho, Wo, ny, nx))) return 0;
  return lowres_tiles(B, Ho, Wo) * ny * nx * K * (int64_t)sizeof(float);
}

// launches the tile kernel of a shape that takes the tile form (a.patches, and a.tile_loss with LOSS, are set)
template <typename Pix, bool LOSS>
int lowres_launch_tiles(LowresArgs<typename Pix::Opt>& a, int K, hipStream_t st) {
  int ny, nx;
  lowres_tile_dims(K, a.Hi, a.Wi, a.Ho, a.Wo, ny, nx);
  lowres_tile_shape(a, a.B, a.Hi, a.Wi, a.Ho, a.Wo, ny, nx);
  const unsigned tiles = (unsigned)lowres_tiles(a.B, a.Ho, a.Wo);
  LOWRES_K_SWITCH(Pix, K, if (KK <= 8) {
                            constexpr int K8 = KK <= 8 ? KK : 8;
                            GDL_SET_MAX_LDS_ONCE((lowres_tile_front_kernel<K8, Pix, LOSS>), 159 * 1024);
                            hipLaunchKernelGGL((lowres_tile_front_kernel<K8, Pix, LOSS>), dim3(tiles), dim3(CT_T),
                                               lowres_tile_lds(K8, ny, nx), st, a);
                          });
  return GDL_OK;
}

// The backward of `a` (lowres_args) in the form asked for: GDL_FOCAL_TILE (an error where the shape or the workspace does not take
// it), GDL_FOCAL_GATHER, or GDL_FOCAL_AUTO = the tile form wherever it can run.
template <typename Pix>
int lowres_bwd(const char* who, LowresArgs<typename Pix::Opt>& a, int K, int form, float* ws, int64_t ws_bytes, hipStream_t st) {
  GDL_CHECK_ARG(form == GDL_FOCAL_AUTO || form == GDL_FOCAL_GATHER || form == GDL_FOCAL_TILE, "%s: unknown form %d", who, form);
  const int64_t need = lowres_bwd_need(K, Pix::ONE_CLASS, a.B, a.Hi, a.Wi, a.Ho, a.Wo);
  const bool can_tile = need > 0 && ws && ws_bytes >= need;
  GDL_CHECK_ARG(form != GDL_FOCAL_TILE || can_tile, "%s: this shape or workspace does not take the tile form", who);
  if (can_tile && form != GDL_FOCAL_GATHER) {
    a.patches = ws;
    int rc = lowres_launch_tiles<Pix, false>(a, K, st);
    if (rc != GDL_OK) return rc;
    rc = lowres_launch_reduce(a, K, st);
    if (rc != GDL_OK) return rc;
  } else {
    const int64_t total = (int64_t)a.B * a.Hi * a.Wi;
    LOWRES_K_SWITCH(Pix, K, hipLaunchKernelGGL((lowres_gather_bwd_kernel<KK, Pix>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                                               st, a));
  }
  GDL_CHECK_LAUNCH(who);
  return GDL_OK;
}

}  // namespace
