// Backward gather of the resized 3x3 convolutions (their forward gather-sum: resize_conv_fwd.hip).  In order: the single-pass VALU
// kernel, the two separable passes (rows, columns), the one-pass matrix-core kernel with its BatchNorm-fused form, then the
// launchers and the gdl_resize_conv3x3_bwd_gather* entry points.
#include "gdl_common.h"
#include "resample_vec.h"
#include <type_traits>

namespace {

// Backward of  y = conv3x3(pad 1)(bilinear_resize(x))  WITHOUT the high-resolution data gradient.
//   y[p] = sum_t W_t (S_t U x)[p]      U = the resize (spatial), S_t = shift by tap t with zero fill (spatial), W_t = channel mix
// U and S_t act on pixels, W_t on channels, so they commute:  dx = sum_t W_t^T G_t  and  dW_t = sum_q G_t[q] (x) x[q]  with
//   G_t = U^T S_t^T dy                  -- nine LOW-resolution maps per output channel.
// Both gradients become GEMMs over the low-resolution pixels (1/16 of the MACs of the full-resolution data / weight
// gradient for a x4 resize).  This kernel is the gather G_t[q] = sum_{p'} U[p', q] dy[p' - t] (p' and p' - t inside the
// image), written as [B, Hi, Wi, 9 * N] with tap block 8 - t (the order of gdl_pack_dgrad's flipped taps, so that the
// existing data-gradient operand applies as a 1x1 convolution).  One block per low-resolution row segment; the
// vertical weights are block-uniform.  f32 accumulation, fixed order, no atomics.
// WXL: the window's horizontal weights live in LDS ([NX][thread]) and the column loop is a runtime loop -- for wide windows
// (x8 resize: NX = 20) the fully unrolled loop with register-held weights spilled.
template <typename V, int VEC, int NX, bool WXL = false>
__global__ __launch_bounds__(256) void resize_conv3x3_bwd_gather_kernel(const void* __restrict__ dy, int Ho, int Wo, int N,
                                                                        void* g, int Hi, int Wi) {
  __shared__ float wxs[WXL ? NX + 4 : 1][WXL ? 256 : 1];
  const int cv = N / VEC;
  const int nblk = gridDim.x * gridDim.y;
  const int id = blockIdx.y * gridDim.x + blockIdx.x;
  const int q8 = nblk >> 3, r8 = nblk & 7, xcd = id & 7, idx = id >> 3;      // XCD-major: neighbouring rows share an L2
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  const int brow = lid / gridDim.x, bx = lid - brow * gridDim.x;
  const int j0 = bx * 256 + threadIdx.x;
  if (j0 >= Wi * cv) return;
  const int b = brow / Hi, iy = brow - b * Hi;
  const int ix = j0 / cv, c = (j0 - ix * cv) * VEC;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  int oy_lo = (int)floorf(((float)iy - 0.5f) / ry - 0.5f) - 1, oy_hi = (int)ceilf(((float)iy + 1.5f) / ry - 0.5f) + 1;
  int ox_lo = (int)floorf(((float)ix - 0.5f) / rx - 0.5f) - 1, ox_hi = (int)ceilf(((float)ix + 1.5f) / rx - 0.5f) + 1;
  oy_lo = oy_lo < 0 ? 0 : oy_lo; ox_lo = ox_lo < 0 ? 0 : ox_lo;
  oy_hi = oy_hi > Ho - 1 ? Ho - 1 : oy_hi; ox_hi = ox_hi > Wo - 1 ? Wo - 1 : ox_hi;
  // horizontal weights of the window columns ox_lo + k (zero beyond the window)
  float wx[WXL ? 1 : NX];
  if constexpr (WXL) {
    // rows 0,1 and NX+2,NX+3 of the LDS table are zero guards: column j reads entries j, j+1, j+2 = window k = j-2, j-1, j
    wxs[0][threadIdx.x] = 0.f; wxs[1][threadIdx.x] = 0.f; wxs[NX + 2][threadIdx.x] = 0.f; wxs[NX + 3][threadIdx.x] = 0.f;
    for (int k = 0; k < NX; ++k) {
      const int ox = ox_lo + k;
      float w = 0.f;
      if (ox <= ox_hi) {
        int x0, x1; float lx;
        src_index2(rx, ox, Wi, x0, x1, lx);
        w = (x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f);
      }
      wxs[k + 2][threadIdx.x] = w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const int ox = ox_lo + k;
      wx[k] = 0.f;
      if (ox <= ox_hi) {
        int x0, x1; float lx;
        src_index2(rx, ox, Wi, x0, x1, lx);
        wx[k] = (x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f);
      }
    }
  }
  auto wyf = [&](int oy) -> float {            // vertical weight U_y[oy, iy]; 0 outside the image / the window
    if (oy < oy_lo || oy > oy_hi) return 0.f;
    int y0, y1; float ly;
    src_index2(ry, oy, Hi, y0, y1, ly);
    return (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
  };
  float acc[9][VEC];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[t][e] = 0.f;
  const int sy_lo = oy_lo > 0 ? oy_lo - 1 : 0, sy_hi = oy_hi < Ho - 1 ? oy_hi + 1 : Ho - 1;
  for (int sy = sy_lo; sy <= sy_hi; ++sy) {
    // source pixel p = (sy, sx) feeds tap (r, s) through p' = p + (r - 1, s - 1)
    const float wr[3] = {wyf(sy - 1), wyf(sy), wyf(sy + 1)};
    if (wr[0] == 0.f && wr[1] == 0.f && wr[2] == 0.f) continue;            // uniform over the block
    const int64_t rowoff = (((int64_t)b * Ho + sy) * Wo) * N + c;
    auto column = [&](int sx, float w0, float w1, float w2) {
      if (sx < 0 || sx >= Wo || (w0 == 0.f && w1 == 0.f && w2 == 0.f)) return;
      float v[VEC];
      V::ld(dy, rowoff + (int64_t)sx * N, v);
      const float wc[3] = {w0, w1, w2};
#pragma unroll
      for (int s3 = 0; s3 < 3; ++s3) {
        float gx[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) gx[e] = wc[s3] * v[e];
#pragma unroll
        for (int r3 = 0; r3 < 3; ++r3)
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[r3 * 3 + s3][e] += wr[r3] * gx[e];
      }
    };
    // p'_x = sx + s - 1 = ox_lo + (j + s - 2): window column index k = j + s - 2
    if constexpr (WXL) {
#pragma unroll 2
      for (int j = 0; j < NX + 2; ++j) column(ox_lo - 1 + j, wxs[j][threadIdx.x], wxs[j + 1][threadIdx.x], wxs[j + 2][threadIdx.x]);
    } else {
#pragma unroll
      for (int j = 0; j < NX + 2; ++j) {
        const float w0 = (j - 2 >= 0 && j - 2 < NX) ? wx[j - 2 < 0 ? 0 : (j - 2 >= NX ? NX - 1 : j - 2)] : 0.f;
        const float w1 = (j - 1 >= 0 && j - 1 < NX) ? wx[j - 1 < 0 ? 0 : (j - 1 >= NX ? NX - 1 : j - 1)] : 0.f;
        const float w2 = (j < NX) ? wx[j >= NX ? NX - 1 : j] : 0.f;
        column(ox_lo - 1 + j, w0, w1, w2);
      }
    }
  }
  const int64_t obase = ((((int64_t)b * Hi + iy) * Wi) + ix) * (9 * (int64_t)N) + c;
#pragma unroll
  for (int t = 0; t < 9; ++t) V::st(g, obase + (int64_t)(8 - t) * N, acc[t]);
}

// The same gather in two separable passes (U = U_y (x) U_x and S_t = S_r (x) S_s, so U^T S_t^T = (U_y^T S_r^T) (x) (U_x^T S_s^T)):
//   pass 1 (rows):    R_r[b, iy, ox] = sum_sy U_y[sy + r - 1, iy] dy[b, sy, ox]          three maps [3][B, Hi, Wo, N]
//   pass 2 (columns): G_(r,s)[b, iy, ix] = sum_sx U_x[sx + s - 1, ix] R_r[b, iy, sx]     nine maps, tap block 8 - (3 r + s)
// One load feeds 3 FMAs per channel in each pass instead of 12 per load over a (rows x columns) window: the single-pass kernel
// is VALU-bound at resize factors of 4 and 8 (1.35 ms for the 1 GB gradient of the neck's x4 level against 0.3 ms of
// memory time); the price is the intermediate (3 / factor of dy's size, written and read once, in dy's dtype).
template <typename V, int VEC>
__global__ __launch_bounds__(256) void resize_conv3x3_bwd_rows_kernel(const void* __restrict__ dy, int Ho, int Wo, int N,
                                                                      void* r3, int Hi, int64_t plane) {
  const int cv = N / VEC;
  const int nblk = gridDim.x * gridDim.y;
  const int id = blockIdx.y * gridDim.x + blockIdx.x;
  const int q8 = nblk >> 3, r8 = nblk & 7, xcd = id & 7, idx = id >> 3;
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  const int brow = lid / gridDim.x, bx = lid - brow * gridDim.x;
  const int j0 = bx * 256 + threadIdx.x;
  if (j0 >= Wo * cv) return;
  const int b = brow / Hi, iy = brow - b * Hi;
  const int ox = j0 / cv, c = (j0 - ox * cv) * VEC;
  const float ry = (float)Hi / (float)Ho;
  int oy_lo = (int)floorf(((float)iy - 0.5f) / ry - 0.5f) - 1, oy_hi = (int)ceilf(((float)iy + 1.5f) / ry - 0.5f) + 1;
  oy_lo = oy_lo < 0 ? 0 : oy_lo;
  oy_hi = oy_hi > Ho - 1 ? Ho - 1 : oy_hi;
  auto wyf = [&](int oy) -> float {
    if (oy < oy_lo || oy > oy_hi) return 0.f;
    int y0, y1; float ly;
    src_index2(ry, oy, Hi, y0, y1, ly);
    return (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
  };
  float acc[3][VEC];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[t][e] = 0.f;
  const int sy_lo = oy_lo > 0 ? oy_lo - 1 : 0, sy_hi = oy_hi < Ho - 1 ? oy_hi + 1 : Ho - 1;
  for (int sy = sy_lo; sy <= sy_hi; ++sy) {
    const float wr[3] = {wyf(sy - 1), wyf(sy), wyf(sy + 1)};
    if (wr[0] == 0.f && wr[1] == 0.f && wr[2] == 0.f) continue;
    float v[VEC];
    V::ld(dy, (((int64_t)b * Ho + sy) * Wo + ox) * N + c, v);
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[t][e] += wr[t] * v[e];
  }
  const int64_t o = (((int64_t)b * Hi + iy) * Wo + ox) * N + c;
#pragma unroll
  for (int t = 0; t < 3; ++t) V::st(r3, o + t * plane, acc[t]);
}

template <typename V, int VEC, int NX, bool WXL>
__global__ __launch_bounds__(256) void resize_conv3x3_bwd_cols_kernel(const void* __restrict__ r3, int Wo, int N, void* g, int Hi,
                                                                      int Wi, int64_t plane) {
  __shared__ float wxs[WXL ? NX + 4 : 1][WXL ? 256 : 1];
  const int cv = N / VEC;
  const int j0 = blockIdx.x * 256 + threadIdx.x;
  if (j0 >= Wi * cv) return;
  const int brow = blockIdx.y;                         // = b * Hi + iy
  const int ix = j0 / cv, c = (j0 - ix * cv) * VEC;
  const float rx = (float)Wi / (float)Wo;
  int ox_lo = (int)floorf(((float)ix - 0.5f) / rx - 0.5f) - 1, ox_hi = (int)ceilf(((float)ix + 1.5f) / rx - 0.5f) + 1;
  ox_lo = ox_lo < 0 ? 0 : ox_lo;
  ox_hi = ox_hi > Wo - 1 ? Wo - 1 : ox_hi;
  auto wxf = [&](int k) -> float {
    const int ox = ox_lo + k;
    if (ox > ox_hi) return 0.f;
    int x0, x1; float lx;
    src_index2(rx, ox, Wi, x0, x1, lx);
    return (x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f);
  };
  float wx[WXL ? 1 : NX];
  if constexpr (WXL) {
    wxs[0][threadIdx.x] = 0.f; wxs[1][threadIdx.x] = 0.f; wxs[NX + 2][threadIdx.x] = 0.f; wxs[NX + 3][threadIdx.x] = 0.f;
    for (int k = 0; k < NX; ++k) wxs[k + 2][threadIdx.x] = wxf(k);
  } else {
#pragma unroll
    for (int k = 0; k < NX; ++k) wx[k] = wxf(k);
  }
  float acc[9][VEC];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[t][e] = 0.f;
  const int64_t rowoff = (int64_t)brow * Wo * N + c;
  auto column = [&](int sx, float w0, float w1, float w2) {
    if (sx < 0 || sx >= Wo || (w0 == 0.f && w1 == 0.f && w2 == 0.f)) return;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      float v[VEC];
      V::ld(r3, rowoff + r * plane + (int64_t)sx * N, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        acc[r * 3 + 0][e] += w0 * v[e];
        acc[r * 3 + 1][e] += w1 * v[e];
        acc[r * 3 + 2][e] += w2 * v[e];
      }
    }
  };
  if constexpr (WXL) {
#pragma unroll 2
    for (int j = 0; j < NX + 2; ++j) column(ox_lo - 1 + j, wxs[j][threadIdx.x], wxs[j + 1][threadIdx.x], wxs[j + 2][threadIdx.x]);
  } else {
#pragma unroll
    for (int j = 0; j < NX + 2; ++j) {
      const float w0 = (j - 2 >= 0 && j - 2 < NX) ? wx[j - 2 < 0 ? 0 : (j - 2 >= NX ? NX - 1 : j - 2)] : 0.f;
      const float w1 = (j - 1 >= 0 && j - 1 < NX) ? wx[j - 1 < 0 ? 0 : (j - 1 >= NX ? NX - 1 : j - 1)] : 0.f;
      const float w2 = (j < NX) ? wx[j >= NX ? NX - 1 : j] : 0.f;
      column(ox_lo - 1 + j, w0, w1, w2);
    }
  }
  const int64_t obase = ((int64_t)brow * Wi + ix) * (9 * (int64_t)N) + c;
#pragma unroll
  for (int t = 0; t < 9; ++t) V::st(g, obase + (int64_t)(8 - t) * N, acc[t]);
}

// ---- the BACKWARD gather on the matrix cores (bf16, N % 64 == 0, factors 2 and 4): G_t = U^T S_t^T dy as ONE pass.
// For a low-resolution pixel q the nine maps are a small dense product that is the same for every channel:
//   G[q, t, n] = sum_p W[p, t] dy[p, n],   p = the (2F + 2)^2 output pixels whose tap positions interpolate from q,
//   W[p, (r, s)] = Uy[py + r - 1, qy] Ux[px + s - 1, qx]   (zero when the position lies outside the output),
// k = 16 * (row of the window) + (column of the window): three (factor 2) or five (factor 4) v_mfma_f32_16x16x32_bf16 steps per
// 16 channels, nine of the sixteen output columns used.  The two-pass kernels above move dy once and an intermediate of 3 / F
// of its size twice (0.93 ms for the neck's x4 level); here dy is staged once per 64 channels into LDS by DMA, the weights are
// products of two small tables, and -- as in the forward kernel (version 2) -- a block walks all channel chunks with the next
// window in flight and everything channel-independent in registers.  One block = four neighbouring pixels of one
// low-resolution row (one per wave).  Output layout = the two-pass kernels': [B, Hi, Wi, 9 N], tap block 8 - t.
//
// BN = true (round 5): the gradient that is gathered is the BatchNorm(+ReLU) backward of the incoming one, formed on the way
// into the LDS -- dy = ga rs (dz [bn(x) > 0] - mean(dz') - xhat mean(dz' xhat)) per element from dz and the convolution output
// x, with four per-channel constants (bn_bwd_coef_kernel).  The separate bn_bwd_dx pass (read dz, read x, write dy: 3 GB at
// the neck's x4 level) and this kernel's read of dy are replaced by one read of dz and x here.  The LDS-DMA cannot transform,
// so this variant stages through registers: a lane always fetches source chunk (lane & 7) -- its eight channels and their
// constants stay in registers for a whole channel step -- and the bank swizzle moves to the LDS side of the write.
struct GatherMArgs {
  const uint16_t* dy;
  uint16_t* g;
  int B, Ho, Wo, N, Hi, Wi;
  const uint16_t* x;      // BN: the convolution output the statistics were taken from, same layout as dy
  const float* coef;      // BN: [N / 8][4][8] = {a, thr, c2, c3} per channel (bn_bwd_coef_kernel)
};

// dy = a * (x a > thr ? dz : 0) - (c2 x + c3):  a = gamma rstd, thr = a mean - beta (-inf without ReLU),
// c2 = a rstd k2, c3 = a k1 - c2 mean with k1 = sum(dz') / P, k2 = sum(dz' xhat) / P   (bn_bwd_dx of norm.hip, refactored)
__global__ __launch_bounds__(256) void bn_bwd_coef_kernel(const float* __restrict__ mean, const float* __restrict__ var,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                          int relu, const float* __restrict__ dgamma_sum,
                                                          const float* __restrict__ dbeta_sum, double inv_p, int N, float* __restrict__ coef) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= N) return;
  const double rs = 1.0 / sqrt((double)var[ch] + (double)eps), a = (double)gamma[ch] * rs;
  const double k1 = (double)dbeta_sum[ch] * inv_p, k2 = (double)dgamma_sum[ch] * inv_p;
  const double c2 = a * k2 * rs, c3 = a * k1 - c2 * (double)mean[ch];
  float* o = coef + (ch >> 3) * 32 + (ch & 7);
  o[0] = (float)a;
  o[8] = relu ? (float)(a * (double)mean[ch] - (double)beta[ch]) : -INFINITY;
  o[16] = (float)c2;
  o[24] = (float)c3;
}

template <int LF, bool BN = false>
__global__ __launch_bounds__(256, 2) void resize_conv3x3_bwd_gather_mfma_kernel(const GatherMArgs a) {
  constexpr int F = 1 << LF, WINB = 2 * F + 2, NKS = WINB / 2, QB = 4;
  constexpr int WCOLS = F * (QB - 1) + WINB;                         // window columns of the block
  constexpr int NROWS = WINB * WCOLS, NPIECES = (NROWS + 7) / 8, MAXP = (NPIECES + 3) / 4;
  constexpr int SLOT = NPIECES * 1024;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* TYb = (float*)smem;                                         // [3][16]      weight of window row for filter row r
  float* TXb = TYb + 48;                                             // [QB][3][16]  the same for columns, per pixel of the block
  unsigned char* tile = smem + 1024;                                 // [QB * 9 rows][128 B]
  unsigned char* ring = tile + 5 * 1024;
  const unsigned lds_ring = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) void*)ring);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nblk = gridDim.x * gridDim.y;
  const int id = blockIdx.y * gridDim.x + blockIdx.x;
  const int q8 = nblk >> 3, r8 = nblk & 7, xcd = id & 7, idx = id >> 3;      // XCD-major: neighbouring rows share an L2
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  const int brow = lid / gridDim.x, cb = lid - brow * gridDim.x;
  const int b = brow / a.Hi, qy = brow - b * a.Hi;
  const int qxb0 = cb * QB;
  const int py0 = F * qy - (F / 2 + 1), pxb0 = F * qxb0 - (F / 2 + 1);
  const float ry = (float)a.Hi / (float)a.Ho, rx = (float)a.Wi / (float)a.Wo;
  if (tid < 48) {
    const int r = tid >> 4, wl = tid & 15;
    float w = 0.f;
    const int pos = py0 + wl + r - 1;
    if (wl < WINB && pos >= 0 && pos < a.Ho && py0 + wl >= 0 && py0 + wl < a.Ho) {
      int y0, y1; float ly;
      src_index2(ry, pos, a.Hi, y0, y1, ly);
      w = (y0 == qy ? 1.f - ly : 0.f) + (y1 == qy ? ly : 0.f);
    }
    TYb[tid] = w;
  }
  if (tid >= 64 && tid < 64 + QB * 48) {
    const int i = tid - 64, j = i / 48, r3 = (i - j * 48) >> 4, wl = i & 15;
    const int qx = qxb0 + j, px = pxb0 + F * j + wl, pos = px + r3 - 1;
    float w = 0.f;
    if (wl < WINB && qx < a.Wi && pos >= 0 && pos < a.Wo && px >= 0 && px < a.Wo) {
      int x0, x1; float lx;
      src_index2(rx, pos, a.Wi, x0, x1, lx);
      w = (x0 == qx ? 1.f - lx : 0.f) + (x1 == qx ? lx : 0.f);
    }
    TXb[i] = w;
  }
  __syncthreads();
  // ---- channel-independent state: weight fragments (B operand: column = tap), fragment addresses, DMA offsets
  const int L = lane & 15, g = lane >> 4;
  const int j = wave;                                                // this wave's pixel of the block
  bf16x8_t wf[NKS];
  int raddr[NKS][2];
  {
    const int r = L / 3, s3 = L - 3 * r;
    float txv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) txv[e] = L < 9 ? TXb[(j * 3 + s3) * 16 + 8 * (g & 1) + e] : 0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int pyl = 2 * ks + (g >> 1);
      const float ty = L < 9 ? TYb[r * 16 + pyl] : 0.f;
      uint32_t pk[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) pk[e] = pack_bf16x2(ty * txv[2 * e], ty * txv[2 * e + 1]);
      wf[ks] = __builtin_bit_cast(bf16x8_t, make_uint4(pk[0], pk[1], pk[2], pk[3]));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int pxl = 8 * (g & 1) + 4 * h + (L >> 2);
        const bool ok = pyl < WINB && pxl < WINB;
        const int R = ok ? pyl * WCOLS + F * j + pxl : 0;            // padding slots: any staged row, their weight is zero
        raddr[ks][h] = R * 128 + (((((L & 3) >> 1) ^ tm_swz(R))) << 4) + (L & 1) * 8;
      }
    }
  }
  unsigned doff[MAXP];
#pragma unroll
  for (int i = 0; i < MAXP; ++i) {
    const int R = (wave + 4 * i) * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ tm_swz(R);
    const int wy = R / WCOLS, wc = R - wy * WCOLS;
    const int py = py0 + wy, px = pxb0 + wc;
    const bool ok = R < NROWS && py >= 0 && py < a.Ho && px >= 0 && px < a.Wo;
    doff[i] = ok ? (unsigned)(((py * a.Wo + px) * a.N) * 2 + chunk * 16) : kTmOob;
  }
  const srd_t srd = make_srd(a.dy + (int64_t)b * a.Ho * a.Wo * a.N, (unsigned)((int64_t)a.Ho * a.Wo * a.N * 2));
  auto issue = [&](int c) {
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
      if (wave + 4 * i < NPIECES) dma16_buf(doff[i], srd, (unsigned)(c * 128), lds_ring + (c & 1) * SLOT + (wave + 4 * i) * 1024);
    }
  };
  // ---- BN: register staging.  Lane = (row lane >> 3 of the piece, source chunk lane & 7)
  typedef __attribute__((ext_vector_type(4))) unsigned gb_u4;
  constexpr int MAXPB = BN ? MAXP : 1;
  unsigned boff[MAXPB], bdst[MAXPB];
  gb_u4 rdz[MAXPB], rxv[MAXPB];
  float ca[8], cthr[8], cc2[8], cc3[8];
  __amdgpu_buffer_rsrc_t rs_dz, rs_x;
  if constexpr (BN) {
    const unsigned img_bytes = (unsigned)((int64_t)a.Ho * a.Wo * a.N * 2);
    rs_dz = __builtin_amdgcn_make_buffer_rsrc((void*)(a.dy + (int64_t)b * a.Ho * a.Wo * a.N), 0, img_bytes, 0x00020000);
    rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)(a.x + (int64_t)b * a.Ho * a.Wo * a.N), 0, img_bytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
      const int R = (wave + 4 * i) * 8 + (lane >> 3);
      const int wy = R / WCOLS, wc = R - wy * WCOLS;
      const int py = py0 + wy, px = pxb0 + wc;
      const bool ok = R < NROWS && py >= 0 && py < a.Ho && px >= 0 && px < a.Wo;
      boff[i] = ok ? (unsigned)(((py * a.Wo + px) * a.N) * 2 + (lane & 7) * 16) : kTmOob;
      bdst[i] = (unsigned)((wave + 4 * i) * 1024 + (lane >> 3) * 128 + (((lane & 7) ^ tm_swz(R)) << 4));
    }
  }
  auto bn_load = [&](int c) {
    if constexpr (BN) {
#pragma unroll
      for (int i = 0; i < MAXP; ++i) {
        if (wave + 4 * i < NPIECES) {
          rdz[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_dz, boff[i], c * 128, 0);
          rxv[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, boff[i], c * 128, 0);
        }
      }
      const float4* cp = (const float4*)(a.coef + ((int64_t)c * 8 + (lane & 7)) * 32);
      const float4 t0 = cp[0], t1 = cp[1], t2 = cp[2], t3 = cp[3], t4 = cp[4], t5 = cp[5], t6 = cp[6], t7 = cp[7];
      ca[0] = t0.x; ca[1] = t0.y; ca[2] = t0.z; ca[3] = t0.w; ca[4] = t1.x; ca[5] = t1.y; ca[6] = t1.z; ca[7] = t1.w;
      cthr[0] = t2.x; cthr[1] = t2.y; cthr[2] = t2.z; cthr[3] = t2.w; cthr[4] = t3.x; cthr[5] = t3.y; cthr[6] = t3.z; cthr[7] = t3.w;
      cc2[0] = t4.x; cc2[1] = t4.y; cc2[2] = t4.z; cc2[3] = t4.w; cc2[4] = t5.x; cc2[5] = t5.y; cc2[6] = t5.z; cc2[7] = t5.w;
      cc3[0] = t6.x; cc3[1] = t6.y; cc3[2] = t6.z; cc3[3] = t6.w; cc3[4] = t7.x; cc3[5] = t7.y; cc3[6] = t7.z; cc3[7] = t7.w;
    }
  };
  auto bn_store = [&](int c) {
    if constexpr (BN) {
#pragma unroll
      for (int i = 0; i < MAXP; ++i) {
        if (wave + 4 * i < NPIECES) {
          const unsigned dzw[4] = {rdz[i].x, rdz[i].y, rdz[i].z, rdz[i].w}, xw[4] = {rxv[i].x, rxv[i].y, rxv[i].z, rxv[i].w};
          uint32_t pk[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float x0 = __uint_as_float(xw[e] << 16), x1 = __uint_as_float(xw[e] & 0xffff0000u);
            const float g0 = __uint_as_float(dzw[e] << 16), g1 = __uint_as_float(dzw[e] & 0xffff0000u);
            const float m0 = x0 * ca[2 * e] > cthr[2 * e] ? g0 : 0.f, m1 = x1 * ca[2 * e + 1] > cthr[2 * e + 1] ? g1 : 0.f;
            const float o0 = fmaf(ca[2 * e], m0, -fmaf(cc2[2 * e], x0, cc3[2 * e]));
            const float o1 = fmaf(ca[2 * e + 1], m1, -fmaf(cc2[2 * e + 1], x1, cc3[2 * e + 1]));
            pk[e] = boff[i] == kTmOob ? 0u : pack_bf16x2(o0, o1);      // out-of-image / padding rows stay zeros, as the DMA leaves them
          }
          *(uint4*)(ring + (c & 1) * SLOT + bdst[i]) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        }
      }
    }
  };
  const int nchunks = a.N >> 6;
  if constexpr (BN) { bn_load(0); bn_store(0); }
  else issue(0);
  for (int c = 0; c < nchunks; ++c) {
    if constexpr (!BN) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                                 // chunk c landed; nobody reads the other slot or the tile
    if (c + 1 < nchunks) {
      if constexpr (BN) bn_load(c + 1);
      else issue(c + 1);
    }
    const unsigned char* stage = ring + (c & 1) * SLOT;
    f32x4_t acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      acc[nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const tm_s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tm_lds_s16x4_ptr)(stage + (raddr[ks][0] ^ (nt << 5))));
        const tm_s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tm_lds_s16x4_ptr)(stage + (raddr[ks][1] ^ (nt << 5))));
        const tm_s16x8_t zv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, zv), wf[ks], acc[nt], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // D[n][t]: lane = (tap L, channels 4 g ..): tile row = pixel * 9 + (8 - tap)
    if (L < 9) {
      const int row = j * 9 + (8 - L);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int ch = 16 * nt + 4 * g;
        *(uint2*)(tile + row * 128 + ((((ch >> 3) ^ (row & 7))) << 4) + (ch & 7) * 2) =
            make_uint2(pack_bf16x2(acc[nt][0], acc[nt][1]), pack_bf16x2(acc[nt][2], acc[nt][3]));
      }
    }
    __syncthreads();
    for (int i = tid; i < QB * 9 * 8; i += 256) {
      const int row = i >> 3, chunk = i & 7;
      const int jq = row / 9, tb = row - jq * 9, qx = qxb0 + jq;
      if (qx < a.Wi) {
        const uint4 v = *(const uint4*)(tile + row * 128 + ((chunk ^ (row & 7)) << 4));
        *(uint4*)(a.g + ((((int64_t)b * a.Hi + qy) * a.Wi + qx) * 9 + tb) * a.N + c * 64 + chunk * 8) = v;
      }
    }
    if (BN && c + 1 < nchunks) bn_store(c + 1);       // into the slot last read in iteration c - 1 (two barriers ago)
  }
}

int g_gather_mfma = 1;     // A/B hook (gdl_debug_set_gather_mfma): 0 = the two-pass / single-pass VALU gathers of the backward

}  // namespace

extern "C" void gdl_debug_set_gather_mfma(int on) { g_gather_mfma = on; }

// matrix-core form of the backward gather; returns false when the shape does not qualify (the caller runs the VALU kernels)
static bool gather_mfma_ok(int dtype, int B, int Ho, int Wo, int N, int Hi, int Wi) {
  if (!g_gather_mfma || dtype != GDL_BF16 || N % 64 != 0 || Hi <= 0 || Wi <= 0) return false;
  const int f = Ho / Hi;
  if (!((f == 2 || f == 4) && Hi * f == Ho && Wi * f == Wo)) return false;
  return (int64_t)B * Hi <= 65535 && (int64_t)Ho * Wo * N * 2 < 0x7ffffff0ll;
}
extern "C" int gdl_resize_conv3x3_bwd_gather_one_pass(int dtype, int B, int Ho, int Wo, int N, int Hi, int Wi) {
  return gather_mfma_ok(dtype, B, Ho, Wo, N, Hi, Wi) ? 1 : 0;
}

template <int LF, bool BN>
static void launch_gather_mfma(dim3 grid, size_t lds, hipStream_t s, const GatherMArgs& a) {
  GDL_SET_MAX_LDS_ONCE((resize_conv3x3_bwd_gather_mfma_kernel<LF, BN>), 160 * 1024);
  hipLaunchKernelGGL((resize_conv3x3_bwd_gather_mfma_kernel<LF, BN>), grid, dim3(256), lds, s, a);
}

static bool gather_mfma_launch(const void* dy, int dtype, int B, int Ho, int Wo, int N, void* g, int Hi, int Wi, hipStream_t s,
                               const void* bn_x = nullptr, const float* bn_coef = nullptr) {
  if (!gather_mfma_ok(dtype, B, Ho, Wo, N, Hi, Wi) || (uintptr_t)dy % 16 || (uintptr_t)g % 16 || (uintptr_t)bn_x % 16) return false;
  const int f = Ho / Hi;
  GatherMArgs a = {(const uint16_t*)dy, (uint16_t*)g, B, Ho, Wo, N, Hi, Wi, (const uint16_t*)bn_x, bn_coef};
  const dim3 grid((unsigned)((Wi + 3) / 4), (unsigned)(B * Hi));
  if (f == 2) {
    constexpr int pieces = (6 * (2 * 3 + 6) + 7) / 8;
    const size_t lds = 6 * 1024 + 2 * pieces * 1024;
    if (bn_x) launch_gather_mfma<1, true>(grid, lds, s, a); else launch_gather_mfma<1, false>(grid, lds, s, a);
  } else {
    constexpr int pieces = (10 * (4 * 3 + 10) + 7) / 8;
    const size_t lds = 6 * 1024 + 2 * pieces * 1024;
    if (bn_x) launch_gather_mfma<2, true>(grid, lds, s, a); else launch_gather_mfma<2, false>(grid, lds, s, a);
  }
  return true;
}

// The gather of gdl_resize_conv3x3_bwd_gather applied to the BatchNorm(+ReLU) backward of dz, without that gradient ever being
// written: see resize_conv3x3_bwd_gather_mfma_kernel<LF, true>.  Only where gdl_resize_conv3x3_bwd_gather_one_pass() says 1.
extern "C" int gdl_resize_conv3x3_bwd_gather_bn(const void* dz, const void* x, int dtype, int B, int Ho, int Wo, int N, void* g, int Hi,
                                                int Wi, const float* mean, const float* var, const float* gamma, const float* beta,
                                                float eps, int relu, const float* dgamma_sum, const float* dbeta_sum, int64_t P_total,
                                                float* coef_ws, gdl_stream_t stream) {
  GDL_CHECK_ARG(dz && x && g && mean && var && gamma && beta && dgamma_sum && dbeta_sum && coef_ws,
                "gdl_resize_conv3x3_bwd_gather_bn: null pointer");
  GDL_CHECK_ARG(B > 0 && Ho > 0 && Wo > 0 && Hi > 0 && Wi > 0 && N > 0 && P_total > 0, "gdl_resize_conv3x3_bwd_gather_bn: bad dims");
  GDL_CHECK_ARG(gather_mfma_ok(dtype, B, Ho, Wo, N, Hi, Wi) && (uintptr_t)dz % 16 == 0 && (uintptr_t)x % 16 == 0 &&
                    (uintptr_t)g % 16 == 0 && (uintptr_t)coef_ws % 16 == 0,
                "gdl_resize_conv3x3_bwd_gather_bn: needs the one-pass matrix-core form (bf16, N %% 64 == 0, factor 2 or 4, "
                "gdl_resize_conv3x3_bwd_gather_one_pass() == 1) and 16-byte aligned pointers");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_bwd_coef_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, mean, var, gamma, beta, eps, relu, dgamma_sum,
                     dbeta_sum, 1.0 / (double)P_total, N, coef_ws);
  const bool ok = gather_mfma_launch(dz, dtype, B, Ho, Wo, N, g, Hi, Wi, s, x, coef_ws);
  GDL_CHECK_ARG(ok, "gdl_resize_conv3x3_bwd_gather_bn: launch refused");
  GDL_CHECK_LAUNCH("gdl_resize_conv3x3_bwd_gather_bn");
  return GDL_OK;
}

extern "C" int64_t gdl_resize_conv3x3_bwd_gather_workspace(int dtype, int B, int Wo, int N, int Hi) {
  if (B <= 0 || Wo <= 0 || N <= 0 || Hi <= 0) return 0;
  return 3ll * B * Hi * Wo * N * (dtype == GDL_BF16 ? 2 : 4);
}

// The instantiation of the gather and columns kernels for a window of nx <= 24 columns: f(NX, WXL), both compile-time constants.
// WXL (the window's weights in LDS: see resize_conv3x3_bwd_gather_kernel) from 20 on; 24 serves the non-integer factors just above 8
// (DOFA-large: 36 -> 292).
template <typename F>
static void for_window_width(int nx, F&& f) {
  if (nx <= 8) f(std::integral_constant<int, 8>{}, std::false_type{});
  else if (nx <= 12) f(std::integral_constant<int, 12>{}, std::false_type{});
  else if (nx <= 20) f(std::integral_constant<int, 20>{}, std::true_type{});
  else f(std::integral_constant<int, 24>{}, std::true_type{});
}

// gdl_resize_conv3x3_bwd_gather (single pass) and gdl_resize_conv3x3_bwd_gather2 (two_pass, with its workspace): the argument
// checks under the entry point's name fn, the one-pass matrix-core form where it applies, else the VALU kernels
static int gather_run(const char* fn, const void* dy, int dtype, int B, int Ho, int Wo, int N, void* g, int Hi, int Wi, bool two_pass,
                      void* ws, int64_t ws_bytes, hipStream_t s) {
  GDL_CHECK_ARG(dy && g && (ws || !two_pass) && B > 0 && Ho > 0 && Wo > 0 && Hi > 0 && Wi > 0, "%s: bad args", fn);
  GDL_CHECK_ARG(dtype == GDL_F32 || dtype == GDL_BF16, "%s: bad dtype", fn);
  const int vec = dtype == GDL_BF16 ? 8 : 4;
  GDL_CHECK_ARG(N % vec == 0 && (uintptr_t)dy % 16 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)ws % 16 == 0,
                "%s: N must be a multiple of the 16-byte vector, pointers 16-byte aligned", fn);
  GDL_CHECK_ARG(!two_pass || ws_bytes >= gdl_resize_conv3x3_bwd_gather_workspace(dtype, B, Wo, N, Hi), "%s: workspace too small", fn);
  GDL_CHECK_ARG((int64_t)B * Hi <= 65535, "%s: B * Hi must fit one grid dimension", fn);
  const int nx = 2 * ((Wo + Wi - 1) / Wi) + 4;             // horizontal output window of one low-resolution pixel, upper bound
  GDL_CHECK_ARG(nx <= 24, "%s: resize factors above 10 are not instantiated", fn);
  if (gather_mfma_launch(dy, dtype, B, Ho, Wo, N, g, Hi, Wi, s)) {      // one pass on the matrix cores: the workspace stays unused
    GDL_CHECK_LAUNCH(fn);
    return GDL_OK;
  }
  const int64_t plane = (int64_t)B * Hi * Wo * N;
  const dim3 grid1((unsigned)((Wo * (N / vec) + 255) / 256), (unsigned)(B * Hi));      // pass 1 (rows) of the two-pass form
  const dim3 grid((unsigned)((Wi * (N / vec) + 255) / 256), (unsigned)(B * Hi));       // the single pass, and pass 2 (columns)
  if (two_pass && dtype == GDL_BF16) hipLaunchKernelGGL((resize_conv3x3_bwd_rows_kernel<V8, 8>), grid1, dim3(256), 0, s, dy, Ho, Wo, N, ws, Hi, plane);
  else if (two_pass) hipLaunchKernelGGL((resize_conv3x3_bwd_rows_kernel<V4<float>, 4>), grid1, dim3(256), 0, s, dy, Ho, Wo, N, ws, Hi, plane);
  for_window_width(nx, [&](auto NX, auto WXL) {
    if (two_pass && dtype == GDL_BF16) hipLaunchKernelGGL((resize_conv3x3_bwd_cols_kernel<V8, 8, NX(), WXL()>), grid, dim3(256), 0, s, ws, Wo, N, g, Hi, Wi, plane);
    else if (two_pass) hipLaunchKernelGGL((resize_conv3x3_bwd_cols_kernel<V4<float>, 4, NX(), WXL()>), grid, dim3(256), 0, s, ws, Wo, N, g, Hi, Wi, plane);
    else if (dtype == GDL_BF16) hipLaunchKernelGGL((resize_conv3x3_bwd_gather_kernel<V8, 8, NX(), WXL()>), grid, dim3(256), 0, s, dy, Ho, Wo, N, g, Hi, Wi);
    else hipLaunchKernelGGL((resize_conv3x3_bwd_gather_kernel<V4<float>, 4, NX(), WXL()>), grid, dim3(256), 0, s, dy, Ho, Wo, N, g, Hi, Wi);
  });
  GDL_CHECK_LAUNCH(fn);
  return GDL_OK;
}

extern "C" int gdl_resize_conv3x3_bwd_gather(const void* dy, int dtype, int B, int Ho, int Wo, int N, void* g, int Hi, int Wi,
                                             gdl_stream_t stream) {
  return gather_run("gdl_resize_conv3x3_bwd_gather", dy, dtype, B, Ho, Wo, N, g, Hi, Wi, false, nullptr, 0, (hipStream_t)stream);
}

// two-pass form of gdl_resize_conv3x3_bwd_gather; ws = gdl_resize_conv3x3_bwd_gather_workspace() bytes (16-byte aligned)
extern "C" int gdl_resize_conv3x3_bwd_gather2(const void* dy, int dtype, int B, int Ho, int Wo, int N, void* g, int Hi, int Wi,
                                              void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  return gather_run("gdl_resize_conv3x3_bwd_gather2", dy, dtype, B, Ho, Wo, N, g, Hi, Wi, true, ws, ws_bytes, (hipStream_t)stream);
}
