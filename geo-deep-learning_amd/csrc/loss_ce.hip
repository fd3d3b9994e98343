// Soft cross-entropy (label smoothing + ignore_index): smp 0.5.0 SoftCrossEntropyLoss (losses/soft_ce.py,
// losses/_functional.py::label_smoothed_nll_loss), the loss of the reference's quick-start notebook
// (notebooks/00_quickstart.ipynb: SoftCrossEntropyLoss(smooth_factor=0.1) on UNet++ / ResNet34).
//
// With e = smooth_factor, K classes, N = B*H*W (ignored pixels counted) and valid_i = [y_i != ignore_index] * [0 <= y_i < K]:
//   L_i      = lse_i - (1 - e) x_{i,y_i} - (e / K) sum_k x_ik
//            = log(sum_k exp(x_ik - m_i)) - (1 - e) (x_{i,y_i} - m_i) - (e / K) sum_k (x_ik - m_i),   m_i = max_k x_ik
//              (the second form is the one evaluated: every term is small where the first one cancels two large ones)
//   dL_i/dx_ik = softmax_k(x_i) - (1 - e) [k == y_i] - e / K
//   loss     = sum_i valid_i L_i / N  (reduction "mean": smp zero-fills the masked entries and calls .mean())  or  sum_i valid_i L_i
// A target outside 0..K-1 that is not ignore_index is treated as ignored (smp's gather would fault on it): the target is only
// ever compared, never used as an index.
//
// Two families, both without float atomics (same input -> same bits on every launch):
//   full resolution  -- NCHW f32 logits: per-workgroup f64 partial sums + a one-workgroup tree (forward); the backward recomputes
//                       the softmax per pixel.  One thread per pixel, every access coalesced over pixels.  K <= 16 is unrolled
//                       over registers; more classes walk the class dimension in a run-time loop (no per-thread array).
//   low resolution   -- the head's NHWC f32 map [B, Hi, Wi, K] and a target at [Ho, Wo]: the bilinear logit of each output pixel is
//                       evaluated on the fly (bilinear_index.h: the expression of gdl_upsample_logits).  The per-pixel gradient
//                       needs no global sums (Dice's does), so a tile kernel can form the loss AND the unscaled partial patches
//                       of d(low) in one pass ("fused" form: the backward is the fixed-order patch reduce times upstream); the
//                       "recompute" form leaves the forward a plain partial-sum pass and runs the tile (K <= 8) or gather kernel
//                       in the backward.
#include <atomic>

#include "gdl_common.h"
#include "bilinear_index.h"

namespace {

struct CeOpt {
  float keep;       // 1 - smooth_factor
  float uni;        // smooth_factor / K
  int has_ignore;
  int64_t ignore;
};

__device__ __forceinline__ bool ce_valid(int64_t t, int K, const CeOpt& o) {
  return (uint64_t)t < (uint64_t)K && !(o.has_ignore && t == o.ignore);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// x[k] -> exp(x[k] - max); returns sum_k of them.  With `L`: the pixel's loss (see the top of the file).
template <int K, bool WITH_LOSS>
__device__ __forceinline__ float ce_softmax(float (&x)[K], int y, const CeOpt& o, float& L) {
  float mx = x[0];
#pragma unroll
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, x[k]);
  float s = 0.f, sx = 0.f, xy = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float d = x[k] - mx;
    sx += d;
    xy = k == y ? d : xy;
    x[k] = expf(d);
    s += x[k];
  }
  if (WITH_LOSS) L = logf(s) - o.keep * xy - o.uni * sx;
  return s;
}

// 256 threads: the workgroup's sum of `acc` (f64, fixed order) -> ws[blockIdx.x]
__device__ __forceinline__ void block256_store_sum(double acc, double* __restrict__ ws) {
  __shared__ double red[4];
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ws[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------------ full resolution
template <int K>
__global__ __launch_bounds__(256) void ce_partial_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B,
                                                         int64_t HW, double* __restrict__ ws, const CeOpt o) {
  const int64_t total = (int64_t)B * HW;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW, p = i - b * HW;
    const int64_t t = target[i];
    float x[K], L;
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = logits[(b * K + k) * HW + p];
    ce_softmax<K, true>(x, (int)t, o, L);
    if (ce_valid(t, K, o)) acc += (double)L;
  }
  block256_store_sum(acc, ws);
}

// any class count: the class dimension in two run-time passes (maximum; sums), the second one out of L1 / L2
__global__ __launch_bounds__(256) void ce_partial_any_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B,
                                                             int K, int64_t HW, double* __restrict__ ws, const CeOpt o) {
  const int64_t total = (int64_t)B * HW;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW, p = i - b * HW;
    const int64_t t = target[i];
    const float* px = logits + b * K * HW + p;
    float mx = px[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, px[(int64_t)k * HW]);
    float s = 0.f, sx = 0.f, xy = 0.f;
    for (int k = 0; k < K; ++k) {
      const float d = px[(int64_t)k * HW] - mx;
      sx += d;
      xy = (int64_t)k == t ? d : xy;
      s += expf(d);
    }
    if (ce_valid(t, K, o)) acc += (double)(logf(s) - o.keep * xy - o.uni * sx);
  }
  block256_store_sum(acc, ws);
}

// one workgroup: sum of the n partials in a fixed order (strided per thread, then a tree), times `scale`
__global__ __launch_bounds__(256) void ce_final_kernel(const double* __restrict__ ws, int n, double scale, float* __restrict__ loss) {
  __shared__ double part[256];
  const int t = threadIdx.x;
  double acc = 0.0;      // (not ordered_sum8: it stages its terms as f32)
#pragma unroll 8
  for (int i = t; i < n; i += 256) acc += ws[i];
  part[t] = acc;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) part[t] += part[t + s];
    __syncthreads();
  }
  if (t == 0) loss[0] = (float)(part[0] * scale);
}

template <int K>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B,
                                                     int64_t HW, const float* __restrict__ upstream, float scale,
                                                     float* __restrict__ dlogits, int accumulate, const CeOpt o) {
  const float c = (upstream ? upstream[0] : 1.f) * scale;
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW, p = i - b * HW;
    const int64_t t = target[i];
    const int y = (int)t;
    float x[K], L;
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = logits[(b * K + k) * HW + p];
    const float inv = 1.f / ce_softmax<K, false>(x, y, o, L);
    const bool valid = ce_valid(t, K, o);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int64_t at = (b * K + k) * HW + p;
      const float v = valid ? c * (x[k] * inv - (k == y ? o.keep : 0.f) - o.uni) : 0.f;      // an ignored pixel: exactly zero
      dlogits[at] = accumulate ? dlogits[at] + v : v;
    }
  }
}

__global__ __launch_bounds__(256) void ce_bwd_any_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B,
                                                         int K, int64_t HW, const float* __restrict__ upstream, float scale,
                                                         float* __restrict__ dlogits, int accumulate, const CeOpt o) {
  const float c = (upstream ? upstream[0] : 1.f) * scale;
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW, p = i - b * HW;
    const int64_t t = target[i];
    const float* px = logits + b * K * HW + p;
    float* pd = dlogits + b * K * HW + p;
    float mx = px[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, px[(int64_t)k * HW]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += expf(px[(int64_t)k * HW] - mx);
    const float inv = 1.f / s;
    const bool valid = ce_valid(t, K, o);
    for (int k = 0; k < K; ++k) {
      const float v = valid ? c * (expf(px[(int64_t)k * HW] - mx) * inv - ((int64_t)k == t ? o.keep : 0.f) - o.uni) : 0.f;
      pd[(int64_t)k * HW] = accumulate ? pd[(int64_t)k * HW] + v : v;
    }
  }
}

// ------------------------------------------------------------------ low resolution
// forward of the recompute form: the partial sums of ce_partial_kernel over the on-the-fly bilinear logits
template <int K>
__global__ __launch_bounds__(256) void ce_lowres_partial_kernel(const float* __restrict__ low, const int64_t* __restrict__ target, int B,
                                                                int Hi, int Wi, int Ho, int Wo, double* __restrict__ ws,
                                                                const CeOpt o) {
  const int64_t total = (int64_t)B * Ho * Wo;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % Wo);
    const int64_t r = i / Wo;
    const int oy = (int)(r % Ho), b = (int)(r / Ho);
    int y0, y1, x0, x1; float ly, lx;
    src_index2(ry, oy, Hi, y0, y1, ly);
    src_index2(rx, ox, Wi, x0, x1, lx);
    const int64_t t = target[i];
    float x[K], L;
    bilinear_logits<K>(low, b, Hi, Wi, y0, y1, x0, x1, ly, lx, x);
    ce_softmax<K, true>(x, (int)t, o, L);
    if (ce_valid(t, K, o)) acc += (double)L;
  }
  block256_store_sum(acc, ws);
}

constexpr int CE_LOWRES_MAX_FACTOR = 64;   // bounds the gather kernel's window: (2 * factor + 4)^2 softmax evaluations per logit vector

// gather form: one thread per LOW-resolution logit vector sums wy * wx * dL/dlogit over the full-resolution pixels that interpolate
// from it, rows then columns in ascending order.  Every class count up to 16; each full-resolution softmax is evaluated once per
// low-resolution neighbour (up to four times).
template <int K>
__global__ __launch_bounds__(256) void ce_lowres_bwd_gather_kernel(const float* __restrict__ low, const int64_t* __restrict__ target,
                                                                   int B, int Hi, int Wi, int Ho, int Wo,
                                                                   const float* __restrict__ upstream, float scale,
                                                                   float* __restrict__ dlow, const CeOpt o) {
  const float c = (upstream ? upstream[0] : 1.f) * scale;
  const int64_t total = (int64_t)B * Hi * Wi;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i % Wi);
    const int64_t r = i / Wi;
    const int iy = (int)(r % Hi), b = (int)(r / Hi);
    int ylo, yhi, xlo, xhi;
    cand_range(iy, ry, Ho, ylo, yhi);
    cand_range(ix, rx, Wo, xlo, xhi);
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
      int y0, y1; float ly;
      src_index2(ry, oy, Hi, y0, y1, ly);
      const float wy = (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
      if (wy == 0.f) continue;
      const int64_t trow = ((int64_t)b * Ho + oy) * Wo;
#pragma unroll 1
      for (int ox = xlo; ox <= xhi; ++ox) {
        int x0, x1; float lx;
        src_index2(rx, ox, Wi, x0, x1, lx);
        const float w = wy * ((x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f));
        if (w == 0.f) continue;
        const int64_t t = target[trow + ox];
        const int y = (int)t;
        float x[K], L;
        bilinear_logits<K>(low, b, Hi, Wi, y0, y1, x0, x1, ly, lx, x);
        const float inv = 1.f / ce_softmax<K, false>(x, y, o, L);
        const bool valid = ce_valid(t, K, o);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float sum = acc[k] + w * (x[k] * inv - (k == y ? o.keep : 0.f) - o.uni);
          acc[k] = valid ? sum : acc[k];      // an ignored pixel adds nothing
        }
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) dlow[i * K + k] = c * acc[k];
  }
}

// tile form (the layout of the Dice tile backward): a workgroup owns a CT_H x CT_W tile of full-resolution pixels,
//   1. dL/dlogit of its pixels (unscaled) -> LDS; with LOSS also the tile's loss sum (f64) -> tile_loss[tile];
//   2. transposed bilinear over rows, 3. over columns -> the tile's partial patch in the workspace.
// ce_lowres_reduce_kernel adds, per low-resolution logit vector, the patches of the (at most four) tiles that touch it in a fixed
// order and applies upstream * scale.  Every full-resolution softmax is evaluated once.  K <= 8 (LDS).
constexpr int CT_H = 32, CT_W = 64, CT_MAXN = 36;
constexpr int CT_T = 1024;

struct CeTile {
  const float* low; const int64_t* target; const float* upstream; double* tile_loss; float* patches; float* dlow;
  int B, Hi, Wi, Ho, Wo, tiles_y, tiles_x, ny_max, nx_max;
  float scale;
  CeOpt o;
};

template <int K, bool LOSS>
__global__ __launch_bounds__(CT_T) void ce_lowres_tile_kernel(const CeTile a) {
  extern __shared__ __attribute__((aligned(16))) float csm[];
  __shared__ double lred[CT_T / 64];
  float* dl = csm;                                   // [K][CT_H][CT_W]
  float* tmp = csm + K * CT_H * CT_W;                // [K][ny_max][CT_W + 1]
  float* wyt = tmp + K * a.ny_max * (CT_W + 1);      // [ny_max][CT_H]  weight of tile row r for low-resolution row iy_lo + j
  float* wxt = wyt + a.ny_max * CT_H;                // [nx_max][CT_W]  the same for columns
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % a.tiles_x, ty = (blockIdx.x / a.tiles_x) % a.tiles_y, b = blockIdx.x / (a.tiles_x * a.tiles_y);
  const int oy0 = ty * CT_H, ox0 = tx * CT_W;
  const int rows = a.Ho - oy0 < CT_H ? a.Ho - oy0 : CT_H, cols = a.Wo - ox0 < CT_W ? a.Wo - ox0 : CT_W;
  const float ry = (float)a.Hi / (float)a.Ho, rx = (float)a.Wi / (float)a.Wo;
  double lacc = 0.0;
  // ---- 1. dL/dlogit of the tile (zeros outside the image and at ignored pixels)
  for (int i = tid; i < CT_H * CT_W; i += CT_T) {
    const int r = i / CT_W, c = i - r * CT_W;
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.f;
    if (r < rows && c < cols) {
      const int oy = oy0 + r, ox = ox0 + c;
      int y0, y1, x0, x1; float ly, lx;
      src_index2(ry, oy, a.Hi, y0, y1, ly);
      src_index2(rx, ox, a.Wi, x0, x1, lx);
      const int64_t t = a.target[((int64_t)b * a.Ho + oy) * a.Wo + ox];
      const int y = (int)t;
      float x[K], L = 0.f;
      bilinear_logits<K>(a.low, b, a.Hi, a.Wi, y0, y1, x0, x1, ly, lx, x);
      const float inv = 1.f / ce_softmax<K, LOSS>(x, y, a.o, L);
      if (ce_valid(t, K, a.o)) {
        if (LOSS) lacc += (double)L;
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = x[k] * inv - (k == y ? a.o.keep : 0.f) - a.o.uni;
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) dl[(k * CT_H + r) * CT_W + c] = v[k];
  }
  if (LOSS) {
    lacc = wave_sum_f64(lacc);
    if ((tid & 63) == 0) lred[tid >> 6] = lacc;
  }
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
  if (LOSS && tid == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < CT_T / 64; ++w) s += lred[w];
    a.tile_loss[blockIdx.x] = s;
  }
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
__global__ __launch_bounds__(256) void ce_lowres_reduce_kernel(const CeTile a) {
  const float cf = (a.upstream ? a.upstream[0] : 1.f) * a.scale;
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

}  // namespace

// ============================================================================ C ABI
static int ce_host_opt(const char* who, int K, float smooth, int has_ignore, int64_t ignore, CeOpt& o) {
  GDL_CHECK_ARG(K >= 1, "%s: K=%d classes", who, K);
  GDL_CHECK_ARG(smooth >= 0.f && smooth <= 1.f, "%s: smooth_factor %g outside [0, 1]", who, (double)smooth);
  o.keep = 1.f - smooth;
  o.uni = smooth / (float)K;
  o.has_ignore = has_ignore != 0;
  o.ignore = ignore;
  return GDL_OK;
}
#define CE_OPT(who, K)                                                                              \
  CeOpt o;                                                                                          \
  { const int st_ = ce_host_opt(who, K, smooth, has_ignore, ignore, o); if (st_ != GDL_OK) return st_; }

// (2048 pixels per workgroup up to 2048 workgroups = eight per CU: a streaming read wants every SIMD full)
static int ce_blocks(int64_t total) {
  int64_t g = (total + 2047) / 2048;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

extern "C" int64_t gdl_soft_ce_workspace(int B, int K, int64_t HW) {
  (void)K;
  return (int64_t)ce_blocks((int64_t)B * HW) * (int64_t)sizeof(double);
}

extern "C" int gdl_soft_ce_fwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, float smooth, int has_ignore,
                               int64_t ignore, int mean, float* loss, void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && loss && ws, "gdl_soft_ce_fwd: null pointer");
  GDL_CHECK_ARG(B > 0 && HW > 0, "gdl_soft_ce_fwd: bad sizes");
  GDL_CHECK_ARG(ws_bytes >= gdl_soft_ce_workspace(B, K, HW) && (uintptr_t)ws % 8 == 0, "gdl_soft_ce_fwd: workspace too small or misaligned");
  CE_OPT("gdl_soft_ce_fwd", K);
  const int64_t total = (int64_t)B * HW;
  const int nblk = ce_blocks(total);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws;
  if (K > 16) {
    hipLaunchKernelGGL(ce_partial_any_kernel, dim3(nblk), dim3(256), 0, s, logits, target, B, K, HW, part, o);
  } else {
    K_SWITCH(K, hipLaunchKernelGGL((ce_partial_kernel<KK>), dim3(nblk), dim3(256), 0, s, logits, target, B, HW, part, o));
  }
  hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, nblk, mean ? 1.0 / (double)total : 1.0, loss);
  GDL_CHECK_LAUNCH("gdl_soft_ce_fwd");
  return GDL_OK;
}

extern "C" int gdl_soft_ce_bwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, float smooth, int has_ignore,
                               int64_t ignore, int mean, const float* upstream, float grad_scale, float* dlogits, int accumulate,
                               gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && dlogits, "gdl_soft_ce_bwd: null pointer");
  GDL_CHECK_ARG(B > 0 && HW > 0, "gdl_soft_ce_bwd: bad sizes");
  CE_OPT("gdl_soft_ce_bwd", K);
  const int64_t total = (int64_t)B * HW;
  const float scale = (float)(mean ? (double)grad_scale / (double)total : (double)grad_scale);
  hipStream_t s = (hipStream_t)stream;
  if (K > 16) {
    hipLaunchKernelGGL(ce_bwd_any_kernel, dim3(grid_for(total)), dim3(256), 0, s, logits, target, B, K, HW, upstream, scale, dlogits, accumulate, o);
  } else {
    K_SWITCH(K, hipLaunchKernelGGL((ce_bwd_kernel<KK>), dim3(grid_for(total)), dim3(256), 0, s, logits, target, B, HW, upstream, scale, dlogits, accumulate, o));
  }
  GDL_CHECK_LAUNCH("gdl_soft_ce_bwd");
  return GDL_OK;
}

// ---- low resolution
#define CE_LOWRES_SHAPE(who)                                                                                                      \
  GDL_CHECK_ARG(B > 0 && Hi > 0 && Wi > 0 && Ho >= Hi && Wo >= Wi, who ": bad sizes (an upsample is expected)");                  \
  GDL_CHECK_ARG((Ho + Hi - 1) / Hi <= CE_LOWRES_MAX_FACTOR && (Wo + Wi - 1) / Wi <= CE_LOWRES_MAX_FACTOR,                         \
                who ": upsampling factors above 64 are not supported");                                                           \
  GDL_CHECK_ARG(K >= 1 && K <= 16, who ": K=%d classes unsupported (1..16)", K)

// (1024 pixels per workgroup, as the Dice low-resolution forward: the scattered loads of the on-the-fly logit are latency bound)
static int ce_lowres_blocks(int64_t total) {
  int64_t g = (total + 1023) / 1024;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

extern "C" int64_t gdl_soft_ce_lowres_workspace(int B, int K, int Ho, int Wo) {
  (void)K;
  return (int64_t)ce_lowres_blocks((int64_t)B * Ho * Wo) * (int64_t)sizeof(double);
}

extern "C" int gdl_soft_ce_lowres_fwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo, float smooth,
                                      int has_ignore, int64_t ignore, int mean, float* loss, void* ws, int64_t ws_bytes,
                                      gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && loss && ws, "gdl_soft_ce_lowres_fwd: null pointer");
  CE_LOWRES_SHAPE("gdl_soft_ce_lowres_fwd");
  GDL_CHECK_ARG(ws_bytes >= gdl_soft_ce_lowres_workspace(B, K, Ho, Wo) && (uintptr_t)ws % 8 == 0,
                "gdl_soft_ce_lowres_fwd: workspace too small or misaligned");
  CE_OPT("gdl_soft_ce_lowres_fwd", K);
  const int64_t total = (int64_t)B * Ho * Wo;
  const int nblk = ce_lowres_blocks(total);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws;
  K_SWITCH(K, hipLaunchKernelGGL((ce_lowres_partial_kernel<KK>), dim3(nblk), dim3(256), 0, s, low, target, B, Hi, Wi, Ho, Wo, part, o));
  hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, nblk, mean ? 1.0 / (double)total : 1.0, loss);
  GDL_CHECK_LAUNCH("gdl_soft_ce_lowres_fwd");
  return GDL_OK;
}

static std::atomic<int> g_ce_tiled{1};
extern "C" void gdl_debug_set_soft_ce_lowres_tiled(int on) { g_ce_tiled = on; }   // A/B hook: 0 = the gather kernel for every class count

static bool ce_tile_dims(int K, int Hi, int Wi, int Ho, int Wo, int& ny_max, int& nx_max) {
  // low-resolution rows / columns one tile side can touch: CT * ratio + 2 (an upper bound for ratios <= 1)
  ny_max = (int)((int64_t)CT_H * Hi / Ho) + 3;
  nx_max = (int)((int64_t)CT_W * Wi / Wo) + 3;
  return K <= 8 && ny_max <= CT_MAXN && nx_max <= CT_MAXN + CT_MAXN;
}
static int64_t ce_tiles(int B, int Ho, int Wo) { return (int64_t)B * ((Ho + CT_H - 1) / CT_H) * ((Wo + CT_W - 1) / CT_W); }

// launches the tile kernel (with or without the loss partials) into `patches`
template <bool LOSS>
static int ce_launch_tiles(CeTile& a, int K, int ny, int nx, hipStream_t st) {
  const unsigned tiles = (unsigned)ce_tiles(a.B, a.Ho, a.Wo);
  K_SWITCH(K, if (KK <= 8) {
                   constexpr int K8 = KK <= 8 ? KK : 8;
                   const size_t lds = ((size_t)K8 * CT_H * CT_W + (size_t)K8 * ny * (CT_W + 1) + (size_t)ny * CT_H + (size_t)nx * CT_W) * sizeof(float);
                   GDL_SET_MAX_LDS_ONCE((ce_lowres_tile_kernel<K8, LOSS>), 159 * 1024);
                   hipLaunchKernelGGL((ce_lowres_tile_kernel<K8, LOSS>), dim3(tiles), dim3(CT_T), lds, st, a);
                 });
  return GDL_OK;
}
static int ce_launch_reduce(const CeTile& a, int K, hipStream_t st) {
  const int64_t total = (int64_t)a.B * a.Hi * a.Wi;
  K_SWITCH(K, if (KK <= 8) hipLaunchKernelGGL((ce_lowres_reduce_kernel<(KK <= 8 ? KK : 8)>), dim3(grid_for(total)), dim3(256), 0, st, a));
  return GDL_OK;
}

// bytes of scratch gdl_soft_ce_lowres_bwd needs (0: none -- the gather kernel)
extern "C" int64_t gdl_soft_ce_lowres_bwd_workspace(int B, int K, int Hi, int Wi, int Ho, int Wo) {
  int ny, nx;
  if (B <= 0 || K < 1 || Hi <= 0 || Wi <= 0 || Ho < Hi || Wo < Wi || !g_ce_tiled || !ce_tile_dims(K, Hi, Wi, Ho, Wo, ny, nx)) return 0;
  return ce_tiles(B, Ho, Wo) * ny * nx * K * (int64_t)sizeof(float);
}

extern "C" int gdl_soft_ce_lowres_bwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo, float smooth,
                                      int has_ignore, int64_t ignore, int mean, const float* upstream, float grad_scale, float* dlow,
                                      float* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && dlow, "gdl_soft_ce_lowres_bwd: null pointer");
  CE_LOWRES_SHAPE("gdl_soft_ce_lowres_bwd");
  CE_OPT("gdl_soft_ce_lowres_bwd", K);
  const int64_t npix = (int64_t)B * Ho * Wo;
  const float scale = (float)(mean ? (double)grad_scale / (double)npix : (double)grad_scale);
  hipStream_t st = (hipStream_t)stream;
  int ny, nx;
  const int64_t need = gdl_soft_ce_lowres_bwd_workspace(B, K, Hi, Wi, Ho, Wo);
  if (need > 0 && ws && ws_bytes >= need && ce_tile_dims(K, Hi, Wi, Ho, Wo, ny, nx)) {
    CeTile a;
    a.low = low; a.target = target; a.upstream = upstream; a.tile_loss = nullptr; a.patches = ws; a.dlow = dlow;
    a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo;
    a.tiles_y = (Ho + CT_H - 1) / CT_H; a.tiles_x = (Wo + CT_W - 1) / CT_W; a.ny_max = ny; a.nx_max = nx;
    a.scale = scale; a.o = o;
    int rc = ce_launch_tiles<false>(a, K, ny, nx, st);
    if (rc != GDL_OK) return rc;
    rc = ce_launch_reduce(a, K, st);
    if (rc != GDL_OK) return rc;
    GDL_CHECK_LAUNCH("gdl_soft_ce_lowres_bwd");
    return GDL_OK;
  }
  const int64_t total = (int64_t)B * Hi * Wi;
  K_SWITCH(K, hipLaunchKernelGGL((ce_lowres_bwd_gather_kernel<KK>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, low, target, B, Hi,
                                    Wi, Ho, Wo, upstream, scale, dlow, o));
  GDL_CHECK_LAUNCH("gdl_soft_ce_lowres_bwd");
  return GDL_OK;
}

// ---- fused form: the forward leaves the unscaled patches of d(low) in `state`; the backward only reduces them.
// state = [tiles f64 loss partials | tiles * ny * nx * K f32 patches]; 0 bytes: the shape does not take this form (K > 8 or a
// resize too close to 1:1 for the tile's LDS tables) and the caller uses gdl_soft_ce_lowres_fwd / _bwd.
extern "C" int64_t gdl_soft_ce_lowres_fused_state(int B, int K, int Hi, int Wi, int Ho, int Wo) {
  int ny, nx;
  if (B <= 0 || K < 1 || Hi <= 0 || Wi <= 0 || Ho < Hi || Wo < Wi || !ce_tile_dims(K, Hi, Wi, Ho, Wo, ny, nx)) return 0;
  if ((Ho + Hi - 1) / Hi > CE_LOWRES_MAX_FACTOR || (Wo + Wi - 1) / Wi > CE_LOWRES_MAX_FACTOR) return 0;
  const int64_t tiles = ce_tiles(B, Ho, Wo);
  return tiles * (int64_t)sizeof(double) + tiles * ny * nx * K * (int64_t)sizeof(float);
}

static int ce_fused_args(const char* who, void* state, int64_t state_bytes, int B, int K, int Hi, int Wi, int Ho, int Wo, CeTile& a) {
  int ny, nx;
  const int64_t need = gdl_soft_ce_lowres_fused_state(B, K, Hi, Wi, Ho, Wo);
  GDL_CHECK_ARG(need > 0 && ce_tile_dims(K, Hi, Wi, Ho, Wo, ny, nx), "%s: this shape does not take the fused form", who);
  GDL_CHECK_ARG(state && state_bytes >= need && (uintptr_t)state % 8 == 0, "%s: state buffer too small or misaligned", who);
  a.tile_loss = (double*)state;
  a.patches = (float*)((char*)state + ce_tiles(B, Ho, Wo) * (int64_t)sizeof(double));
  a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo;
  a.tiles_y = (Ho + CT_H - 1) / CT_H; a.tiles_x = (Wo + CT_W - 1) / CT_W; a.ny_max = ny; a.nx_max = nx;
  return GDL_OK;
}

extern "C" int gdl_soft_ce_lowres_fused_fwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo,
                                            float smooth, int has_ignore, int64_t ignore, int mean, float* loss, void* state,
                                            int64_t state_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && loss, "gdl_soft_ce_lowres_fused_fwd: null pointer");
  CE_LOWRES_SHAPE("gdl_soft_ce_lowres_fused_fwd");
  CE_OPT("gdl_soft_ce_lowres_fused_fwd", K);
  CeTile a;
  int rc = ce_fused_args("gdl_soft_ce_lowres_fused_fwd", state, state_bytes, B, K, Hi, Wi, Ho, Wo, a);
  if (rc != GDL_OK) return rc;
  a.low = low; a.target = target; a.upstream = nullptr; a.dlow = nullptr; a.scale = 1.f; a.o = o;
  hipStream_t st = (hipStream_t)stream;
  rc = ce_launch_tiles<true>(a, K, a.ny_max, a.nx_max, st);
  if (rc != GDL_OK) return rc;
  const int64_t npix = (int64_t)B * Ho * Wo;
  hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(256), 0, st, (const double*)a.tile_loss, (int)ce_tiles(B, Ho, Wo),
                     mean ? 1.0 / (double)npix : 1.0, loss);
  GDL_CHECK_LAUNCH("gdl_soft_ce_lowres_fused_fwd");
  return GDL_OK;
}

extern "C" int gdl_soft_ce_lowres_fused_bwd(const void* state, int64_t state_bytes, int B, int K, int Hi, int Wi, int Ho, int Wo, int mean,
                                            const float* upstream, float grad_scale, float* dlow, gdl_stream_t stream) {
  GDL_CHECK_ARG(dlow, "gdl_soft_ce_lowres_fused_bwd: null pointer");
  CE_LOWRES_SHAPE("gdl_soft_ce_lowres_fused_bwd");
  CeTile a;
  const int rc = ce_fused_args("gdl_soft_ce_lowres_fused_bwd", const_cast<void*>(state), state_bytes, B, K, Hi, Wi, Ho, Wo, a);
  if (rc != GDL_OK) return rc;
  const int64_t npix = (int64_t)B * Ho * Wo;
  a.low = nullptr; a.target = nullptr; a.upstream = upstream; a.dlow = dlow;
  a.scale = (float)(mean ? (double)grad_scale / (double)npix : (double)grad_scale);
  a.o = CeOpt{1.f, 0.f, 0, 0};
  const int rc2 = ce_launch_reduce(a, K, (hipStream_t)stream);
  if (rc2 != GDL_OK) return rc2;
  GDL_CHECK_LAUNCH("gdl_soft_ce_lowres_fused_bwd");
  return GDL_OK;
}
