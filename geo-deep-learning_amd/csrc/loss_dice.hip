// Dice, Jaccard and Tversky losses (smp 0.5.0 losses/dice.py, jaccard.py, tversky.py): one set of pixel kernels and the three
// per-class sums [I | S | N], at full resolution, straight from the low-resolution head map, and in binary mode.
#include <atomic>
#include <cmath>

#include "gdl_common.h"
#include "bilinear_index.h"
#include "lowres_tile.h"

namespace {

// ------------------------------------------------------------------ Dice loss (smp multiclass)
// The constructor options of smp's DiceLoss (losses/dice.py) beyond the defaults:
//   ignore_index -- template flag IGN of the per-pixel kernels: a pixel whose target equals `ignore` (compared as int64, before the
//                   cast to int) adds nothing to the three sums and gets a zero gradient.  IGN = false is the code as it was.
//   smooth, log_loss, classes -- DiceCoef: they only change how the per-class sums become the loss (dice_final_kernel) and the two
//                   per-class gradient coefficients (dice_coeffs); `plain` (smooth == 0, no log, every class) selects the original
//                   expressions so that the defaults stay bit-identical.
// The Jaccard and Tversky losses (gdl_overlap_*) are other functions of the same three sums: `overlap` selects
//   score_c = (I_c + smooth) / max(I_c + alpha (S_c - I_c) + beta (N_c - I_c) + smooth, eps)      (Jaccard: alpha = beta = 1)
// and loss = m^gamma, m = the class mean of L(score_c).  Only dice_final_kernel and dice_coeffs read these fields: every pixel
// pass is shared with Dice.
struct DiceCoef {
  float smooth;
  uint32_t cls;     // bit k: class k takes part in the mean
  int nsel;         // number of set bits (the mean's divisor)
  int log_loss;
  int plain;
  int overlap;      // 0: Dice.  1: the score above (plain == 0)
  float alpha, beta, gamma;
};

// d(m^gamma)/dm = gamma m^(gamma-1) from the sums (K <= 21 scores: cheaper than a device scalar carried from forward to backward).
// DEFINED AS 0 for m <= 0 when gamma != 1: torch gives inf (gamma < 1) and nan further down the chain for a perfect prediction.
template <int K>
__device__ __forceinline__ float overlap_focal_factor(const float* __restrict__ sums, float eps, const DiceCoef o) {
  if (o.gamma == 1.f) return 1.f;
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float I = sums[k], num = I + o.smooth;
    const float den = I + o.alpha * (sums[K + k] - I) + o.beta * (sums[2 * K + k] - I) + o.smooth;
    const float score = num / (den > eps ? den : eps);
    const float l = o.log_loss ? -logf(score > eps ? score : eps) : 1.f - score;
    m += (sums[2 * K + k] > 0.f && ((o.cls >> k) & 1u)) ? l : 0.f;
  }
  m /= (float)o.nsel;
  return m > 0.f ? o.gamma * powf(m, o.gamma - 1.f) : 0.f;
}

// dL/dp_c = ca[c]*[y==c] + cb[c] from sums = [I | S | N]:  loss_c = L(score_c), score_c = (2 I_c + smooth) / max(S_c + N_c + smooth, eps),
// L(s) = 1 - s or -log(max(s, eps)); weight [N_c > 0] * [c selected] / nsel.  `up` = upstream * grad_scale.
template <int K>
__device__ __forceinline__ void dice_coeffs(const float* __restrict__ sums, float eps, float up, const DiceCoef o, float (&ca)[K],
                                            float (&cb)[K]) {
  if (o.plain) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float I = sums[k], card = sums[K + k] + sums[2 * K + k];
      const bool on = sums[2 * K + k] > 0.f && card > eps;
      ca[k] = on ? -2.f / (K * card) * up : 0.f;
      cb[k] = on ? 2.f * I / (K * card * card) * up : 0.f;
    }
  } else if (o.overlap) {
    // score = N / D, N = I + smooth, D = I + alpha (S - I) + beta (Y - I) + smooth:  dD/dI = 1 - alpha - beta, dD/dS = alpha, so
    // d score / dp = [y==c] (D - N dD/dI) / D^2 - N alpha / D^2; a clamped D is a constant (cb = 0), as in the Dice branch below
    const float w = up / (float)o.nsel * overlap_focal_factor<K>(sums, eps, o);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float I = sums[k], num = I + o.smooth;
      const float den = I + o.alpha * (sums[K + k] - I) + o.beta * (sums[2 * K + k] - I) + o.smooth;
      const bool clamped = !(den > eps);
      const float denc = clamped ? eps : den, score = num / denc;
      float f = (sums[2 * K + k] > 0.f && ((o.cls >> k) & 1u)) ? -w : 0.f;
      if (o.log_loss) f = score > eps ? f / score : 0.f;
      ca[k] = clamped ? f / denc : f * (denc - num * (1.f - o.alpha - o.beta)) / (denc * denc);
      cb[k] = clamped ? 0.f : -f * num * o.alpha / (denc * denc);
    }
  } else {
    const float w = up / (float)o.nsel;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float num = 2.f * sums[k] + o.smooth, den = sums[K + k] + sums[2 * K + k] + o.smooth;
      const bool clamped = !(den > eps);
      const float denc = clamped ? eps : den, score = num / denc;
      float f = (sums[2 * K + k] > 0.f && ((o.cls >> k) & 1u)) ? -w : 0.f;      // w_c * [N_c > 0] * L'(score) * up
      if (o.log_loss) f = score > eps ? f / score : 0.f;
      ca[k] = f * 2.f / denc;
      cb[k] = clamped ? 0.f : -f * num / (denc * denc);
    }
  }
}

// pass 1: per-block partial sums of I_c = sum p_c*[y==c], S_c = sum p_c, N_c = count(y==c)
template <int K, bool IGN>
__global__ __launch_bounds__(256) void dice_partial_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                           int B, int64_t HW, float* __restrict__ ws, int64_t ignore) {
  __shared__ float red[4][3 * K];
  const int64_t total = (int64_t)B * HW;
  float I[K], S[K], Nc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) I[k] = S[k] = Nc[k] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if (IGN && target[i] == ignore) continue;
    const int64_t b = i / HW, p = i - b * HW;
    float x[K], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) { x[k] = logits[(b * K + k) * HW + p]; mx = fmaxf(mx, x[k]); }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { x[k] = expf(x[k] - mx); s += x[k]; }
    const float inv = 1.f / s;
    const int y = (int)target[i];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float pk = x[k] * inv;
      S[k] += pk;
      if (y == k) { I[k] += pk; Nc[k] += 1.f; }
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float a = wave_sum(I[k]), bsum = wave_sum(S[k]), c = wave_sum(Nc[k]);
    if (lane == 0) { red[wv][k] = a; red[wv][K + k] = bsum; red[wv][2 * K + k] = c; }
  }
  __syncthreads();
  if (threadIdx.x < 3 * K)
    ws[(int64_t)blockIdx.x * 3 * K + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

template <int K>
__global__ __launch_bounds__(256) void dice_final_kernel(const float* __restrict__ ws, int nblk, float eps,
                                                         float* __restrict__ sums, float* __restrict__ loss, const DiceCoef o) {
  __shared__ double part[4][64];
  __shared__ double tot[64];
  const int t = threadIdx.x, v = t & 63, grp = t >> 6;   // 4 groups of 64 value slots (3K <= 48)
  static_assert(3 * K <= 64, "dice_final_kernel: at most 21 classes");
  double s = 0;
  if (v < 3 * K) s = ordered_sum8<double>(grp, nblk, 4, [&](int i) { return ws[(int64_t)i * 3 * K + v]; });   // same order, 8 loads in flight
  part[grp][v] = s;
  __syncthreads();
  if (t < 3 * K) {
    double r = 0;
    for (int g = 0; g < 4; ++g) r += part[g][t];
    tot[t] = r;
    sums[t] = (float)r;
  }
  __syncthreads();
  if (t == 0 && o.plain) {
    double l = 0;
    for (int k = 0; k < K; ++k) {
      const double I = tot[k], card = tot[K + k] + tot[2 * K + k];
      const double dice = 2.0 * I / (card > eps ? card : eps);
      if (tot[2 * K + k] > 0) l += 1.0 - dice;
    }
    loss[0] = (float)(l / K);
  } else if (t == 0 && o.overlap) {
    double l = 0;
    for (int k = 0; k < K; ++k) {
      if (!((o.cls >> k) & 1u) || !(tot[2 * K + k] > 0)) continue;
      const double I = tot[k], num = I + o.smooth;
      const double den = I + (double)o.alpha * (tot[K + k] - I) + (double)o.beta * (tot[2 * K + k] - I) + o.smooth;
      const double score = num / (den > eps ? den : eps);
      l += o.log_loss ? -log(score > eps ? score : (double)eps) : 1.0 - score;
    }
    const double m = l / o.nsel;
    loss[0] = (float)(o.gamma == 1.f ? m : (m > 0 ? pow(m, (double)o.gamma) : 0.0));      // m <= 0: overlap_focal_factor
  } else if (t == 0) {
    double l = 0;
    for (int k = 0; k < K; ++k) {
      if (!((o.cls >> k) & 1u) || !(tot[2 * K + k] > 0)) continue;
      const double num = 2.0 * tot[k] + o.smooth, den = tot[K + k] + tot[2 * K + k] + o.smooth;
      const double score = num / (den > eps ? den : eps);
      l += o.log_loss ? -log(score > eps ? score : (double)eps) : 1.0 - score;
    }
    loss[0] = (float)(l / o.nsel);
  }
}

// pass 2: dL/dlogits; sums = [I | S | N] as produced above
template <int K, bool IGN>
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                       int B, int64_t HW, const float* __restrict__ sums, float eps,
                                                       const float* __restrict__ upstream, float grad_scale,
                                                       float* __restrict__ dlogits, int accumulate, int64_t ignore,
                                                       const DiceCoef o) {
  float ca[K], cb[K];  // dL/dp_c = ca[c]*[y==c] + cb[c]
  const float up = (upstream ? upstream[0] : 1.f) * grad_scale;
  dice_coeffs<K>(sums, eps, up, o, ca, cb);
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW, p = i - b * HW;
    float x[K], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) { x[k] = logits[(b * K + k) * HW + p]; mx = fmaxf(mx, x[k]); }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { x[k] = expf(x[k] - mx); s += x[k]; }
    const float inv = 1.f / s;
    const int y = (int)target[i];
    float g[K], dot = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      x[k] *= inv;
      g[k] = cb[k] + (y == k ? ca[k] : 0.f);
      dot += x[k] * g[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int64_t o = (b * K + k) * HW + p;
      float v = x[k] * (g[k] - dot);
      if (IGN && target[i] == ignore) v = 0.f;      // an ignored pixel: exactly zero in every class
      dlogits[o] = accumulate ? dlogits[o] + v : v;
    }
  }
}

// ------------------------------------------------------------------ Dice loss straight from the LOW-resolution logits (round 5)
// The training step only needs the loss and its gradient, not the [B, K, 512, 512] f32 logits: per head the tail was
// upsample (write 168 MB) -> dice partial (read 235 MB) -> dice backward (read 235, write 168) -> transposed upsample in two passes
// (read 168 ...), 350 us per head and two heads per step (dofa.py:89-105, segmentation_dofa.py:226-229).  Both kernels below
// evaluate the bilinear logit of a full-resolution pixel on the fly from the [B, Hi, Wi, K] f32 map the 1x1 head wrote (13 MB at
// batch 32: L2 / MALL resident), with the SAME expression as upsample_logits_kernel:
//   forward  -- the three per-class sums of dice_partial_kernel, same workgroup count and pixel order (the same partial sums);
//   backward -- one thread per LOW-resolution logit vector gathers wy * wx * dL/dlogit over the full-resolution pixels that
//               interpolate from it (softmax and Dice coefficients recomputed there): d(low) in one pass, f32, fixed order.
template <int K, bool IGN>
__global__ __launch_bounds__(256) void dice_lowres_partial_kernel(const float* __restrict__ low, const int64_t* __restrict__ target,
                                                                  int B, int Hi, int Wi, int Ho, int Wo, float* __restrict__ ws,
                                                                  int64_t ignore) {
  __shared__ float red[4][3 * K];
  const int64_t total = (int64_t)B * Ho * Wo;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  float I[K], S[K], Nc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) I[k] = S[k] = Nc[k] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % Wo);
    const int64_t t = i / Wo;
    const int oy = (int)(t % Ho), b = (int)(t / Ho);
    int y0, y1, x0, x1; float ly, lx;
    src_index2(ry, oy, Hi, y0, y1, ly);
    src_index2(rx, ox, Wi, x0, x1, lx);
    float x[K], mx = -INFINITY;
    bilinear_logits<K>(low, b, Hi, Wi, y0, y1, x0, x1, ly, lx, x);
#pragma unroll
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, x[k]);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { x[k] = expf(x[k] - mx); s += x[k]; }
    const float inv = 1.f / s;
    const int y = (int)target[i];
    if (IGN && target[i] == ignore) continue;      // (tested here, not at the top: the target load goes out with the logit loads)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float pk = x[k] * inv;
      S[k] += pk;
      if (y == k) { I[k] += pk; Nc[k] += 1.f; }
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float a = wave_sum(I[k]), bsum = wave_sum(S[k]), c = wave_sum(Nc[k]);
    if (lane == 0) { red[wv][k] = a; red[wv][K + k] = bsum; red[wv][2 * K + k] = c; }
  }
  __syncthreads();
  if (threadIdx.x < 3 * K)
    ws[(int64_t)blockIdx.x * 3 * K + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

constexpr int DICE_LOWRES_MAX_FACTOR = 64;   // (every loop below is a run-time loop; the bound only keeps the K > 8 gather kernel's
                                             // window -- (2 * factor + 4)^2 softmax evaluations per low-resolution logit -- finite)

template <int K, bool IGN>
__global__ __launch_bounds__(256) void dice_lowres_bwd_kernel(const float* __restrict__ low, const int64_t* __restrict__ target, int B,
                                                              int Hi, int Wi, int Ho, int Wo, const float* __restrict__ sums,
                                                              float eps, const float* __restrict__ upstream, float grad_scale,
                                                              float* __restrict__ dlow, int64_t ignore, const DiceCoef o) {
  float ca[K], cb[K];  // dL/dp_c = ca[c]*[y==c] + cb[c]   (dice_bwd_kernel)
  const float up = (upstream ? upstream[0] : 1.f) * grad_scale;
  dice_coeffs<K>(sums, eps, up, o, ca, cb);
  const int64_t total = (int64_t)B * Hi * Wi;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i % Wi);
    const int64_t t = i / Wi;
    const int iy = (int)(t % Hi), b = (int)(t / Hi);
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
      // (runtime loop, indices recomputed per column: holding the window's columns in registers -- 4 x 16 values -- and unrolling
      // cost 208 registers = two waves per SIMD for a kernel that lives on L1 / L2 latency)
#pragma unroll 1
      for (int ox = xlo; ox <= xhi; ++ox) {
        int x0, x1; float lx;
        src_index2(rx, ox, Wi, x0, x1, lx);
        const float w = wy * ((x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f));
        if (w == 0.f) continue;
        float x[K], mx = -INFINITY;
        bilinear_logits<K>(low, b, Hi, Wi, y0, y1, x0, x1, ly, lx, x);
#pragma unroll
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, x[k]);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) { x[k] = expf(x[k] - mx); s += x[k]; }
        const float inv = 1.f / s;
        const int64_t t = target[trow + ox];
        const int y = (int)t;
        float g[K], dot = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          x[k] *= inv;
          g[k] = cb[k] + (y == k ? ca[k] : 0.f);
          dot += x[k] * g[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float sum = acc[k] + w * (x[k] * (g[k] - dot));
          acc[k] = (IGN && t == ignore) ? acc[k] : sum;      // an ignored pixel adds nothing
        }
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) dlow[i * K + k] = acc[k];
  }
}

// The same gradient with every full-resolution pixel's softmax evaluated ONCE (the gather kernel above evaluates it once per
// low-resolution logit that interpolates into it: four times, 272 us at batch 32 -- no faster than the three launches it replaced).
// A workgroup owns a DT_H x DT_W tile of full-resolution pixels:
//   1. dL/dlogit of its pixels -> LDS (K x 2048 floats);
//   2. transposed bilinear, rows: tmp[k][iy][c] = sum over the tile's rows of wy(row -> iy) dl[k][row][c] for the low-resolution rows
//      the tile touches (LDS);
//   3. columns: part[k][iy][ix] = sum_c wx(c -> ix) tmp[k][iy][c] -> the tile's partial patch in the workspace.
// dice_lowres_bwd_reduce_kernel then adds, per low-resolution logit, the patches of the (at most four) tiles that touch it, in a
// fixed order.  No atomics, f32, deterministic.  K <= 8 (LDS); more classes take the gather kernel.
constexpr int DT_H = 32, DT_W = 64, DT_MAXN = 36;     // tile; bound on the low-resolution rows / columns one tile side can touch
constexpr int DT_T = 1024;    // threads per tile: two pixels each.  With 256 (eight pixels each, LDS allowing two workgroups per CU =
                              // two waves per SIMD) phase 1 was a chain of eight L2 round trips per thread: 215 us at batch 32

struct DiceTile {
  const float* low; const int64_t* target; const float* sums; const float* upstream; float* ws; float* dlow;
  int B, Hi, Wi, Ho, Wo, tiles_y, tiles_x, ny_max, nx_max;
  float eps, grad_scale;
  int64_t ignore;
  DiceCoef o;
};

template <int K, bool IGN>
__global__ __launch_bounds__(DT_T) void dice_lowres_bwd_tile_kernel(const DiceTile a) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  float* dl = dsm;                                   // [K][DT_H][DT_W]
  float* tmp = dsm + K * DT_H * DT_W;                // [K][ny_max][DT_W + 1]  (+1: phase 3's threads differ in j at equal c)
  float* wyt = tmp + K * a.ny_max * (DT_W + 1);      // [ny_max][DT_H]  weight of tile row r for low-resolution row iy_lo + j
  float* wxt = wyt + a.ny_max * DT_H;                // [nx_max][DT_W]  the same for columns
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % a.tiles_x, ty = (blockIdx.x / a.tiles_x) % a.tiles_y, b = blockIdx.x / (a.tiles_x * a.tiles_y);
  const int oy0 = ty * DT_H, ox0 = tx * DT_W;
  const int rows = a.Ho - oy0 < DT_H ? a.Ho - oy0 : DT_H, cols = a.Wo - ox0 < DT_W ? a.Wo - ox0 : DT_W;
  const float ry = (float)a.Hi / (float)a.Ho, rx = (float)a.Wi / (float)a.Wo;
  float ca[K], cb[K];
  const float up = (a.upstream ? a.upstream[0] : 1.f) * a.grad_scale;
  dice_coeffs<K>(a.sums, a.eps, up, a.o, ca, cb);
  // ---- 1. dL/dlogit of the tile (zeros outside the image)
  for (int i = tid; i < DT_H * DT_W; i += DT_T) {
    const int r = i / DT_W, c = i - r * DT_W;
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.f;
    if (r < rows && c < cols) {
      const int oy = oy0 + r, ox = ox0 + c;
      int y0, y1, x0, x1; float ly, lx;
      src_index2(ry, oy, a.Hi, y0, y1, ly);
      src_index2(rx, ox, a.Wi, x0, x1, lx);
      float x[K], mx = -INFINITY;
      bilinear_logits<K>(a.low, b, a.Hi, a.Wi, y0, y1, x0, x1, ly, lx, x);
#pragma unroll
      for (int k = 0; k < K; ++k) mx = fmaxf(mx, x[k]);
      float sden = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) { x[k] = expf(x[k] - mx); sden += x[k]; }
      const float inv = 1.f / sden;
      const int64_t t = a.target[((int64_t)b * a.Ho + oy) * a.Wo + ox];
      const int y = (int)t;
      float g[K], dot = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        x[k] *= inv;
        g[k] = cb[k] + (y == k ? ca[k] : 0.f);
        dot += x[k] * g[k];
      }
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = (IGN && t == a.ignore) ? 0.f : x[k] * (g[k] - dot);      // an ignored pixel: zero
    }
#pragma unroll
    for (int k = 0; k < K; ++k) dl[(k * DT_H + r) * DT_W + c] = v[k];
  }
  // the low-resolution rows iy_lo .. iy_hi / columns ix_lo .. ix_hi this tile touches, and the two 1-D weight tables
  int iy_lo, iy_hi, ix_lo, ix_hi;
  touched_range(ry, oy0, oy0 + rows - 1, a.Hi, iy_lo, iy_hi);
  touched_range(rx, ox0, ox0 + cols - 1, a.Wi, ix_lo, ix_hi);
  const int ny = iy_hi - iy_lo + 1, nx = ix_hi - ix_lo + 1;
  for (int i = tid; i < ny * DT_H; i += DT_T) {
    const int j = i / DT_H, r = i - j * DT_H;
    float wv = 0.f;
    if (r < rows) {
      int y0, y1; float ly;
      src_index2(ry, oy0 + r, a.Hi, y0, y1, ly);
      wv = (y0 == iy_lo + j ? 1.f - ly : 0.f) + (y1 == iy_lo + j ? ly : 0.f);
    }
    wyt[i] = wv;
  }
  for (int i = tid; i < nx * DT_W; i += DT_T) {
    const int q = i / DT_W, c = i - q * DT_W;
    float wv = 0.f;
    if (c < cols) {
      int x0, x1; float lx;
      src_index2(rx, ox0 + c, a.Wi, x0, x1, lx);
      wv = (x0 == ix_lo + q ? 1.f - lx : 0.f) + (x1 == ix_lo + q ? lx : 0.f);
    }
    wxt[i] = wv;
  }
  __syncthreads();
  // ---- 2. rows
  for (int i = tid; i < ny * DT_W; i += DT_T) {
    const int j = i / DT_W, c = i - j * DT_W;
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    // (only the tile rows that can interpolate from low-resolution row iy_lo + j: 2 / ratio + 3 of the 32 -- same terms, same order)
    int r_lo, r_hi;
    cand_range(iy_lo + j, ry, a.Ho, r_lo, r_hi);
    r_lo = r_lo - oy0 < 0 ? 0 : r_lo - oy0;
    r_hi = r_hi - oy0 > rows - 1 ? rows - 1 : r_hi - oy0;
    for (int r = r_lo; r <= r_hi; ++r) {
      const float wy = wyt[j * DT_H + r];
      if (wy != 0.f) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += wy * dl[(k * DT_H + r) * DT_W + c];
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) tmp[(k * a.ny_max + j) * (DT_W + 1) + c] = acc[k];
  }
  __syncthreads();
  // ---- 3. columns -> the tile's partial patch [ny_max][nx_max][K] in the workspace (entries beyond ny / nx are never read)
  float* patch = a.ws + (int64_t)blockIdx.x * a.ny_max * a.nx_max * K;
  for (int i = tid; i < ny * nx; i += DT_T) {
    const int j = i / nx, q = i - j * nx;
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    int c_lo, c_hi;
    cand_range(ix_lo + q, rx, a.Wo, c_lo, c_hi);
    c_lo = c_lo - ox0 < 0 ? 0 : c_lo - ox0;
    c_hi = c_hi - ox0 > cols - 1 ? cols - 1 : c_hi - ox0;
    for (int c = c_lo; c <= c_hi; ++c) {
      const float wx = wxt[q * DT_W + c];
      if (wx != 0.f) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += wx * tmp[(k * a.ny_max + j) * (DT_W + 1) + c];
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) patch[(j * a.nx_max + q) * K + k] = acc[k];
  }
}

template <int K>
__global__ __launch_bounds__(256) void dice_lowres_bwd_reduce_kernel(const DiceTile a) {
  const int64_t total = (int64_t)a.B * a.Hi * a.Wi;
  const float ry = (float)a.Hi / (float)a.Ho, rx = (float)a.Wi / (float)a.Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i % a.Wi);
    const int64_t t = i / a.Wi;
    const int iy = (int)(t % a.Hi), b = (int)(t / a.Hi);
    int ylo, yhi, xlo, xhi;
    cand_range(iy, ry, a.Ho, ylo, yhi);              // full-resolution rows / columns that can interpolate from (iy, ix)
    cand_range(ix, rx, a.Wo, xlo, xhi);
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    for (int ty = ylo / DT_H; ty <= yhi / DT_H; ++ty) {
      const int oy0 = ty * DT_H, rows = a.Ho - oy0 < DT_H ? a.Ho - oy0 : DT_H;
      int iy_lo, iy_hi;
      touched_range(ry, oy0, oy0 + rows - 1, a.Hi, iy_lo, iy_hi);
      if (iy < iy_lo || iy > iy_hi) continue;
      for (int tx = xlo / DT_W; tx <= xhi / DT_W; ++tx) {
        const int ox0 = tx * DT_W, cols = a.Wo - ox0 < DT_W ? a.Wo - ox0 : DT_W;
        int ix_lo, ix_hi;
        touched_range(rx, ox0, ox0 + cols - 1, a.Wi, ix_lo, ix_hi);
        if (ix < ix_lo || ix > ix_hi) continue;
        const float* patch = a.ws + ((int64_t)(b * a.tiles_y + ty) * a.tiles_x + tx) * a.ny_max * a.nx_max * K;
        const float* src = patch + ((iy - iy_lo) * a.nx_max + (ix - ix_lo)) * K;
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += src[k];
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) a.dlow[i * K + k] = acc[k];
  }
}

// ------------------------------------------------------------------ Dice loss (smp binary)
// smp DiceLoss(mode="binary") (configs/unetplus_config_RGB.yaml: num_classes 1): p = exp(logsigmoid(x)), one class,
// sums over dims (batch, pixels); the target is used as a 0/1 weight.  Partials have the multiclass layout with K = 1
// ([I | S | N]) so dice_final_kernel<1> finishes them (loss * [sum y > 0], mean over the single class).
template <bool IGN>
__global__ __launch_bounds__(256) void dice_binary_partial_kernel(const float* __restrict__ logits,
                                                                  const int64_t* __restrict__ target, int64_t total,
                                                                  float* __restrict__ ws, int64_t ignore) {
  __shared__ float red[4][3];
  float I = 0.f, S = 0.f, Nc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if (IGN && target[i] == ignore) continue;
    const float x = logits[i];
    // exp(logsigmoid(x)) with logsigmoid(x) = min(x, 0) - log1p(exp(-|x|)), as torch computes it
    const float p = expf(fminf(x, 0.f) - log1pf(expf(-fabsf(x))));
    const float y = (float)target[i];
    I += p * y; S += p; Nc += y;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float a = wave_sum(I), b = wave_sum(S), c = wave_sum(Nc);
  if (lane == 0) { red[wv][0] = a; red[wv][1] = b; red[wv][2] = c; }
  __syncthreads();
  if (threadIdx.x < 3)
    ws[(int64_t)blockIdx.x * 3 + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

template <bool IGN>
__global__ __launch_bounds__(256) void dice_binary_bwd_kernel(const float* __restrict__ logits,
                                                              const int64_t* __restrict__ target, int64_t total,
                                                              const float* __restrict__ sums, float eps,
                                                              const float* __restrict__ upstream, float grad_scale,
                                                              float* __restrict__ dlogits, int accumulate, int64_t ignore,
                                                              const DiceCoef o) {
  const float up = (upstream ? upstream[0] : 1.f) * grad_scale;
  float ca, cb;                                              // dL/dp = ca * y + cb
  if (o.plain) {
    const float I = sums[0], card = sums[1] + sums[2];
    const bool on = sums[2] > 0.f && card > eps;
    ca = on ? -2.f / card * up : 0.f;
    cb = on ? 2.f * I / (card * card) * up : 0.f;
  } else {
    float a1[1], b1[1];
    dice_coeffs<1>(sums, eps, up, o, a1, b1);
    ca = a1[0]; cb = b1[0];
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if (IGN && target[i] == ignore) {
      if (!accumulate) dlogits[i] = 0.f;
      continue;
    }
    const float x = logits[i];
    const float p = expf(fminf(x, 0.f) - log1pf(expf(-fabsf(x))));
    const float v = (cb + ca * (float)target[i]) * p * (1.f - p);
    dlogits[i] = accumulate ? dlogits[i] + v : v;
  }
}

// ------------------------------------------------------------------ Dice loss (smp binary) straight from the LOW-resolution logits
// The one-class head (configs/unetplus_config_RGB.yaml: num_classes 1) hands out low [B, Hi, Wi, 1]; the training step resized it to
// [B, 1, Ho, Wo] f32 (dofa.py:89-105), read that in dice_binary_partial_kernel and dice_binary_bwd_kernel and sent the gradient back
// through the transposed resize.  The kernels below evaluate the bilinear logit of a full-resolution pixel on the fly (bilinear_index.h:
// the expression of upsample_logits_kernel), p = exp(logsigmoid(x)) as dice_binary_partial_kernel writes it, and the target as a 0/1
// weight:
//   forward  -- the sums [I | S | N] in the K = 1 layout (dice_final_kernel<1> finishes them), workgroups and pixel order of
//               dice_lowres_partial_kernel;
//   backward -- dL/dx = (cb + ca y) p (1 - p) with dice_coeffs<1> at upstream 1 (DiceBinaryPix), in the gather or the tile form of
//               lowres_tile.h at K = 1.  Both forms multiply by upstream * grad_scale once, at the end.
// No float atomics: the same input gives the same bits on every launch.
template <bool IGN>
__global__ __launch_bounds__(256) void dice_binary_lowres_partial_kernel(const float* __restrict__ low, const int64_t* __restrict__ target,
                                                                         int B, int Hi, int Wi, int Ho, int Wo, float* __restrict__ ws,
                                                                         int64_t ignore) {
  __shared__ float red[4][3];
  const int64_t total = (int64_t)B * Ho * Wo;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  float I = 0.f, S = 0.f, Nc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % Wo);
    const int64_t r = i / Wo;
    const int oy = (int)(r % Ho), b = (int)(r / Ho);
    int y0, y1, x0, x1; float ly, lx;
    src_index2(ry, oy, Hi, y0, y1, ly);
    src_index2(rx, ox, Wi, x0, x1, lx);
    float x[1];
    bilinear_logits<1>(low, b, Hi, Wi, y0, y1, x0, x1, ly, lx, x);
    const int64_t t = target[i];
    if (IGN && t == ignore) continue;      // (tested here, not at the top: the target load goes out with the logit loads)
    const float p = expf(fminf(x[0], 0.f) - log1pf(expf(-fabsf(x[0]))));
    const float y = (float)t;
    I += p * y; S += p; Nc += y;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float a = wave_sum(I), b = wave_sum(S), c = wave_sum(Nc);
  if (lane == 0) { red[wv][0] = a; red[wv][1] = b; red[wv][2] = c; }
  __syncthreads();
  if (threadIdx.x < 3)
    ws[(int64_t)blockIdx.x * 3 + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// the backward's policy of lowres_tile.h
struct DiceBinaryOpt {
  const float* sums;
  float eps;
  int64_t ignore;
  DiceCoef o;
};
template <bool IGN>
struct DiceBinaryPix {
  typedef DiceBinaryOpt Opt;
  typedef int64_t Target;
  static constexpr bool ONE_CLASS = true;
  float ca[1], cb[1];      // dL/dp = ca * y + cb at upstream 1
  int64_t ignore;
  __device__ DiceBinaryPix(const DiceBinaryOpt& d, int) : ignore(d.ignore) { dice_coeffs<1>(d.sums, d.eps, 1.f, d.o, ca, cb); }
  __device__ bool valid(int64_t t) const { return !(IGN && t == ignore); }
  __device__ void grad(const float (&x)[1], int64_t t, float (&g)[1]) const {
    const float p = expf(fminf(x[0], 0.f) - log1pf(expf(-fabsf(x[0]))));
    g[0] = (cb[0] + ca[0] * (float)t) * p * (1.f - p);
  }
};

}  // namespace

// ============================================================================ C ABI
static int dice_blocks(int64_t total) {
  int64_t g = (total + 2047) / 2048;
  return (int)(g < 1 ? 1 : (g > 512 ? 512 : g));
}

extern "C" int64_t gdl_dice_loss_workspace(int B, int K, int64_t HW) {
  return (int64_t)dice_blocks((int64_t)B * HW) * 3 * K * sizeof(float);
}

// gdl_dice_options (host) -> the kernels' arguments.  Null = smp's defaults.
struct DiceHostOpt { bool ign; int64_t ignore; DiceCoef o; };
// `classes` -> the bit mask and the mean's divisor (none listed: all K)
static int dice_host_classes(const int* classes, int num_classes, int K, const char* who, DiceCoef& o) {
  o.cls = K >= 32 ? 0xffffffffu : ((1u << K) - 1u); o.nsel = K;
  if (num_classes < 0 || (num_classes > 0 && !classes)) {
    gdl_set_error("%s: bad class list", who);
    return GDL_ERR_INVALID;
  }
  if (num_classes > 0) {
    o.cls = 0;
    for (int i = 0; i < num_classes; ++i) {
      const int c = classes[i];
      if (c < 0 || c >= K || ((o.cls >> c) & 1u)) {
        gdl_set_error("%s: classes must be distinct indices in 0..%d (got %d)", who, K - 1, c);
        return GDL_ERR_INVALID;
      }
      o.cls |= 1u << c;
    }
    o.nsel = num_classes;
  }
  return GDL_OK;
}
static int dice_host_opt(const gdl_dice_options* opt, int K, const char* who, DiceHostOpt& h) {
  const uint32_t all = K >= 32 ? 0xffffffffu : ((1u << K) - 1u);
  h.ign = false; h.ignore = 0;
  h.o.smooth = 0.f; h.o.cls = all; h.o.nsel = K; h.o.log_loss = 0; h.o.plain = 1;
  h.o.overlap = 0; h.o.alpha = h.o.beta = 0.5f; h.o.gamma = 1.f;
  if (!opt) return GDL_OK;
  { const int st = dice_host_classes(opt->classes, opt->num_classes, K, who, h.o); if (st != GDL_OK) return st; }
  h.ign = opt->has_ignore_index != 0; h.ignore = opt->ignore_index;
  h.o.smooth = opt->smooth; h.o.log_loss = opt->log_loss != 0;
  h.o.plain = h.o.smooth == 0.f && !h.o.log_loss && h.o.cls == all;
  return GDL_OK;
}
// gdl_overlap_options (host) -> the same arguments with DiceCoef::overlap set.  Jaccard is the Tversky score with alpha = beta = 1
// and no focal exponent; it takes no ignore_index (smp's JaccardLoss has none).
static int overlap_host_opt(const gdl_overlap_options* opt, int K, const char* who, DiceHostOpt& h) {
  if (!opt) { gdl_set_error("%s: null options", who); return GDL_ERR_INVALID; }
  { const int st = dice_host_classes(opt->classes, opt->nclasses, K, who, h.o); if (st != GDL_OK) return st; }
  h.o.plain = 0; h.o.overlap = 1;
  h.o.smooth = opt->smooth; h.o.log_loss = opt->log_loss != 0;
  if (!std::isfinite(h.o.smooth)) { gdl_set_error("%s: smooth must be finite", who); return GDL_ERR_INVALID; }
  if (opt->kind == GDL_OVERLAP_JACCARD) {
    if (opt->has_ignore) { gdl_set_error("%s: the Jaccard loss takes no ignore_index", who); return GDL_ERR_INVALID; }
    h.ign = false; h.ignore = 0;
    h.o.alpha = h.o.beta = 1.f; h.o.gamma = 1.f;
  } else if (opt->kind == GDL_OVERLAP_TVERSKY) {
    if (!(opt->alpha >= 0.f && opt->beta >= 0.f && opt->gamma > 0.f) || !std::isfinite(opt->alpha) || !std::isfinite(opt->beta) ||
        !std::isfinite(opt->gamma)) {
      gdl_set_error("%s: finite alpha, beta >= 0 and gamma > 0 expected (got %g, %g, %g)", who, opt->alpha, opt->beta, opt->gamma);
      return GDL_ERR_INVALID;
    }
    h.ign = opt->has_ignore != 0; h.ignore = opt->ignore_index;
    h.o.alpha = opt->alpha; h.o.beta = opt->beta; h.o.gamma = opt->gamma;
  } else {
    gdl_set_error("%s: unknown kind %d (GDL_OVERLAP_JACCARD or GDL_OVERLAP_TVERSKY)", who, opt->kind);
    return GDL_ERR_INVALID;
  }
  return GDL_OK;
}
// What an entry point received: gdl_dice_options (null = smp's defaults) or gdl_overlap_options.  The *_run helpers serve both
// families and resolve() it after their pointer / size checks, as the Dice entry points always did.
struct DiceFamilyOpt {
  const gdl_dice_options* dice = nullptr;
  const gdl_overlap_options* overlap = nullptr;
  bool is_overlap;
  explicit DiceFamilyOpt(const gdl_dice_options* o) : dice(o), is_overlap(false) {}
  explicit DiceFamilyOpt(const gdl_overlap_options* o) : overlap(o), is_overlap(true) {}
  int resolve(int K, const char* who, DiceHostOpt& h) const {
    return is_overlap ? overlap_host_opt(overlap, K, who, h) : dice_host_opt(dice, K, who, h);
  }
};
// launch `kernel<..., IG>` with IG = IGN (two instantiations; IG = false is the code without the test)
#define IGN_SWITCH(IGN, ...)                                                  \
  if (IGN) { constexpr bool IG = true; __VA_ARGS__; } else { constexpr bool IG = false; __VA_ARGS__; }

// The launches behind the gdl_dice_*_opt_* and gdl_overlap_* entry points; `who` names the caller in error messages.
static int dice_fwd_run(const float* logits, const int64_t* target, int B, int K, int64_t HW, float eps, DiceFamilyOpt opt,
                        const char* who, float* sums, float* loss, float* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && sums && loss && ws, "%s: null pointer", who);
  GDL_CHECK_ARG(ws_bytes >= gdl_dice_loss_workspace(B, K, HW), "%s: workspace too small", who);
  DiceHostOpt h;
  if (const int st = opt.resolve(K, who, h); st != GDL_OK) return st;
  const int nblk = dice_blocks((int64_t)B * HW);
  hipStream_t s = (hipStream_t)stream;
  K_SWITCH(K, IGN_SWITCH(h.ign, hipLaunchKernelGGL((dice_partial_kernel<KK, IG>), dim3(nblk), dim3(256), 0, s, logits, target, B, HW, ws, h.ignore));
              hipLaunchKernelGGL((dice_final_kernel<KK>), dim3(1), dim3(256), 0, s, ws, nblk, eps, sums, loss, h.o));
  GDL_CHECK_LAUNCH(who);
  return GDL_OK;
}
extern "C" int gdl_dice_loss_opt_fwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, float eps,
                                     const gdl_dice_options* opt, float* sums, float* loss, float* ws, int64_t ws_bytes,
                                     gdl_stream_t stream) {
  return dice_fwd_run(logits, target, B, K, HW, eps, DiceFamilyOpt(opt), "gdl_dice_loss_fwd", sums, loss, ws, ws_bytes, stream);
}
extern "C" int gdl_dice_loss_fwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, float eps,
                                 float* sums, float* loss, float* ws, int64_t ws_bytes, gdl_stream_t stream) {
  return gdl_dice_loss_opt_fwd(logits, target, B, K, HW, eps, nullptr, sums, loss, ws, ws_bytes, stream);
}
extern "C" int gdl_overlap_loss_fwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, float eps,
                                    const gdl_overlap_options* opt, float* sums, float* loss, float* ws, int64_t ws_bytes,
                                    gdl_stream_t stream) {
  return dice_fwd_run(logits, target, B, K, HW, eps, DiceFamilyOpt(opt), "gdl_overlap_loss_fwd", sums, loss, ws, ws_bytes, stream);
}

// (four times the workgroups of dice_partial_kernel: the scattered 4-byte loads of the on-the-fly bilinear logit are a chain of L2
// round trips per pixel, and 512 workgroups = two waves per SIMD do not cover it)
static int dice_lowres_blocks(int64_t total) {
  int64_t g = (total + 1023) / 1024;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}
extern "C" int64_t gdl_dice_loss_lowres_workspace(int B, int K, int Ho, int Wo) {
  return (int64_t)dice_lowres_blocks((int64_t)B * Ho * Wo) * 3 * K * sizeof(float);
}

// Dice loss (multiclass) of bilinear(low -> [Ho, Wo]) against target [B, Ho, Wo] WITHOUT the full-resolution logits: low = the
// [B, Hi, Wi, K] f32 map gdl_head_1x1 writes.  sums / loss as gdl_dice_loss_fwd; workspace of gdl_dice_loss_lowres_workspace(B, K, Ho,
// Wo) bytes.  Upsampling factors up to 64 per direction.
static int dice_lowres_fwd_run(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo, float eps,
                               DiceFamilyOpt opt, const char* who, float* sums, float* loss, float* ws, int64_t ws_bytes,
                               gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && sums && loss && ws, "%s: null pointer", who);
  GDL_CHECK_ARG(B > 0 && Hi > 0 && Wi > 0 && Ho >= Hi && Wo >= Wi, "%s: bad sizes (an upsample is expected)", who);
  GDL_CHECK_ARG((Ho + Hi - 1) / Hi <= DICE_LOWRES_MAX_FACTOR && (Wo + Wi - 1) / Wi <= DICE_LOWRES_MAX_FACTOR,
                "%s: upsampling factors above 64 are not supported", who);
  GDL_CHECK_ARG(ws_bytes >= gdl_dice_loss_lowres_workspace(B, K, Ho, Wo), "%s: workspace too small", who);
  DiceHostOpt h;
  if (const int st = opt.resolve(K, who, h); st != GDL_OK) return st;
  const int nblk = dice_lowres_blocks((int64_t)B * Ho * Wo);
  hipStream_t s = (hipStream_t)stream;
  K_SWITCH(K, IGN_SWITCH(h.ign, hipLaunchKernelGGL((dice_lowres_partial_kernel<KK, IG>), dim3(nblk), dim3(256), 0, s, low, target, B, Hi, Wi, Ho, Wo, ws, h.ignore));
              hipLaunchKernelGGL((dice_final_kernel<KK>), dim3(1), dim3(256), 0, s, ws, nblk, eps, sums, loss, h.o));
  GDL_CHECK_LAUNCH(who);
  return GDL_OK;
}
extern "C" int gdl_dice_loss_lowres_opt_fwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo,
                                            float eps, const gdl_dice_options* opt, float* sums, float* loss, float* ws,
                                            int64_t ws_bytes, gdl_stream_t stream) {
  return dice_lowres_fwd_run(low, target, B, K, Hi, Wi, Ho, Wo, eps, DiceFamilyOpt(opt), "gdl_dice_loss_lowres_fwd", sums, loss, ws, ws_bytes, stream);
}
extern "C" int gdl_dice_loss_lowres_fwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo, float eps,
                                        float* sums, float* loss, float* ws, int64_t ws_bytes, gdl_stream_t stream) {
  return gdl_dice_loss_lowres_opt_fwd(low, target, B, K, Hi, Wi, Ho, Wo, eps, nullptr, sums, loss, ws, ws_bytes, stream);
}
extern "C" int gdl_overlap_loss_lowres_fwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo,
                                           float eps, const gdl_overlap_options* opt, float* sums, float* loss, float* ws,
                                           int64_t ws_bytes, gdl_stream_t stream) {
  return dice_lowres_fwd_run(low, target, B, K, Hi, Wi, Ho, Wo, eps, DiceFamilyOpt(opt), "gdl_overlap_loss_lowres_fwd", sums, loss, ws, ws_bytes, stream);
}

static std::atomic<int> g_dice_tiled{1};
extern "C" void gdl_debug_set_dice_lowres_tiled(int on) { g_dice_tiled = on; }   // A/B hook: 0 = the gather kernel for every class count

static bool dice_tile_dims(int K, int Hi, int Wi, int Ho, int Wo, int& ny_max, int& nx_max) {
  // low-resolution rows / columns one tile side can touch: DT * ratio + 2 (an upper bound for ratios <= 1)
  ny_max = (int)((int64_t)DT_H * Hi / Ho) + 3;
  nx_max = (int)((int64_t)DT_W * Wi / Wo) + 3;
  return g_dice_tiled && K <= 8 && ny_max <= DT_MAXN && nx_max <= DT_MAXN + DT_MAXN;
}

// bytes of scratch gdl_dice_loss_lowres_bwd needs (0: none -- the gather kernel)
extern "C" int64_t gdl_dice_loss_lowres_bwd_workspace(int B, int K, int Hi, int Wi, int Ho, int Wo) {
  int ny, nx;
  if (B <= 0 || Hi <= 0 || Wi <= 0 || Ho < Hi || Wo < Wi || !dice_tile_dims(K, Hi, Wi, Ho, Wo, ny, nx)) return 0;
  const int64_t tiles = (int64_t)B * ((Ho + DT_H - 1) / DT_H) * ((Wo + DT_W - 1) / DT_W);
  return tiles * ny * nx * K * (int64_t)sizeof(float);
}

// d loss / d low [B, Hi, Wi, K] (f32, overwritten) from the sums of the forward; upstream (device scalar, may be null) * grad_scale
// multiplies the gradient.  ws: gdl_dice_loss_lowres_bwd_workspace() bytes (may be null when that is 0).
static int dice_lowres_bwd_run(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo, float eps,
                               DiceFamilyOpt opt, const char* who, const float* sums, const float* upstream, float grad_scale,
                               float* dlow, float* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && sums && dlow, "%s: null pointer", who);
  GDL_CHECK_ARG(B > 0 && Hi > 0 && Wi > 0 && Ho >= Hi && Wo >= Wi, "%s: bad sizes", who);
  GDL_CHECK_ARG((Ho + Hi - 1) / Hi <= DICE_LOWRES_MAX_FACTOR && (Wo + Wi - 1) / Wi <= DICE_LOWRES_MAX_FACTOR,
                "%s: upsampling factors above 64 are not supported", who);
  DiceHostOpt h;
  if (const int st = opt.resolve(K, who, h); st != GDL_OK) return st;
  {
    int ny, nx;
    const int64_t need = gdl_dice_loss_lowres_bwd_workspace(B, K, Hi, Wi, Ho, Wo);
    if (need > 0 && ws && ws_bytes >= need && dice_tile_dims(K, Hi, Wi, Ho, Wo, ny, nx)) {
      DiceTile a;
      a.low = low; a.target = target; a.sums = sums; a.upstream = upstream; a.ws = ws; a.dlow = dlow;
      a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo;
      a.tiles_y = (Ho + DT_H - 1) / DT_H; a.tiles_x = (Wo + DT_W - 1) / DT_W; a.ny_max = ny; a.nx_max = nx;
      a.eps = eps; a.grad_scale = grad_scale; a.ignore = h.ignore; a.o = h.o;
      const unsigned tiles = (unsigned)(B * a.tiles_y * a.tiles_x);
      const int64_t total = (int64_t)B * Hi * Wi;
      hipStream_t st = (hipStream_t)stream;
      K_SWITCH(K, if (KK <= 8) {
                    const size_t lds = ((size_t)KK * DT_H * DT_W + (size_t)KK * ny * (DT_W + 1) + (size_t)ny * DT_H + (size_t)nx * DT_W) * sizeof(float);
                    IGN_SWITCH(h.ign, GDL_SET_MAX_LDS_ONCE((dice_lowres_bwd_tile_kernel<(KK <= 8 ? KK : 8), IG>), 160 * 1024);
                               hipLaunchKernelGGL((dice_lowres_bwd_tile_kernel<(KK <= 8 ? KK : 8), IG>), dim3(tiles), dim3(DT_T), lds, st, a));
                    hipLaunchKernelGGL((dice_lowres_bwd_reduce_kernel<(KK <= 8 ? KK : 8)>), dim3(grid_for(total)), dim3(256), 0, st, a);
                  });
      GDL_CHECK_LAUNCH(who);
      return GDL_OK;
    }
  }
  const int64_t total = (int64_t)B * Hi * Wi;
  K_SWITCH(K, IGN_SWITCH(h.ign, hipLaunchKernelGGL((dice_lowres_bwd_kernel<KK, IG>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, low,
                                            target, B, Hi, Wi, Ho, Wo, sums, eps, upstream, grad_scale, dlow, h.ignore, h.o)));
  GDL_CHECK_LAUNCH(who);
  return GDL_OK;
}
extern "C" int gdl_dice_loss_lowres_opt_bwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo,
                                            float eps, const gdl_dice_options* opt, const float* sums, const float* upstream,
                                            float grad_scale, float* dlow, float* ws, int64_t ws_bytes, gdl_stream_t stream) {
  return dice_lowres_bwd_run(low, target, B, K, Hi, Wi, Ho, Wo, eps, DiceFamilyOpt(opt), "gdl_dice_loss_lowres_bwd", sums, upstream, grad_scale, dlow,
                             ws, ws_bytes, stream);
}
extern "C" int gdl_dice_loss_lowres_bwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo, float eps,
                                        const float* sums, const float* upstream, float grad_scale, float* dlow, float* ws,
                                        int64_t ws_bytes, gdl_stream_t stream) {
  return gdl_dice_loss_lowres_opt_bwd(low, target, B, K, Hi, Wi, Ho, Wo, eps, nullptr, sums, upstream, grad_scale, dlow, ws, ws_bytes,
                                      stream);
}
extern "C" int gdl_overlap_loss_lowres_bwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo,
                                           float eps, const gdl_overlap_options* opt, const float* sums, const float* upstream,
                                           float grad_scale, float* dlow, float* ws, int64_t ws_bytes, gdl_stream_t stream) {
  return dice_lowres_bwd_run(low, target, B, K, Hi, Wi, Ho, Wo, eps, DiceFamilyOpt(opt), "gdl_overlap_loss_lowres_bwd", sums, upstream, grad_scale,
                             dlow, ws, ws_bytes, stream);
}

static int dice_bwd_run(const float* logits, const int64_t* target, int B, int K, int64_t HW, float eps, DiceFamilyOpt opt,
                        const char* who, const float* sums, const float* upstream, float grad_scale, float* dlogits,
                        int accumulate, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && sums && dlogits, "%s: null pointer", who);
  DiceHostOpt h;
  if (const int st = opt.resolve(K, who, h); st != GDL_OK) return st;
  const int64_t total = (int64_t)B * HW;
  K_SWITCH(K, IGN_SWITCH(h.ign, hipLaunchKernelGGL((dice_bwd_kernel<KK, IG>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, logits, target, B, HW, sums, eps, upstream, grad_scale, dlogits, accumulate, h.ignore, h.o)));
  GDL_CHECK_LAUNCH(who);
  return GDL_OK;
}
extern "C" int gdl_dice_loss_opt_bwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, float eps,
                                     const gdl_dice_options* opt, const float* sums, const float* upstream, float grad_scale,
                                     float* dlogits, int accumulate, gdl_stream_t stream) {
  return dice_bwd_run(logits, target, B, K, HW, eps, DiceFamilyOpt(opt), "gdl_dice_loss_bwd", sums, upstream, grad_scale, dlogits, accumulate, stream);
}
extern "C" int gdl_dice_loss_bwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, float eps,
                                 const float* sums, const float* upstream, float grad_scale, float* dlogits,
                                 int accumulate, gdl_stream_t stream) {
  return gdl_dice_loss_opt_bwd(logits, target, B, K, HW, eps, nullptr, sums, upstream, grad_scale, dlogits, accumulate, stream);
}
extern "C" int gdl_overlap_loss_bwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, float eps,
                                    const gdl_overlap_options* opt, const float* sums, const float* upstream, float grad_scale,
                                    float* dlogits, int accumulate, gdl_stream_t stream) {
  return dice_bwd_run(logits, target, B, K, HW, eps, DiceFamilyOpt(opt), "gdl_overlap_loss_bwd", sums, upstream, grad_scale, dlogits, accumulate, stream);
}

static int dice_binary_fwd_run(const float* logits, const int64_t* target, int64_t total, float eps, DiceFamilyOpt opt,
                               const char* who, float* sums, float* loss, float* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && sums && loss && ws, "%s: null pointer", who);
  const int nblk = dice_blocks(total);
  GDL_CHECK_ARG(ws_bytes >= (int64_t)nblk * 3 * (int64_t)sizeof(float), "%s: workspace too small", who);
  DiceHostOpt h;
  if (const int st = opt.resolve(1, who, h); st != GDL_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  IGN_SWITCH(h.ign, hipLaunchKernelGGL((dice_binary_partial_kernel<IG>), dim3(nblk), dim3(256), 0, s, logits, target, total, ws, h.ignore));
  hipLaunchKernelGGL((dice_final_kernel<1>), dim3(1), dim3(256), 0, s, ws, nblk, eps, sums, loss, h.o);
  GDL_CHECK_LAUNCH(who);
  return GDL_OK;
}
extern "C" int gdl_dice_binary_loss_opt_fwd(const float* logits, const int64_t* target, int64_t total, float eps,
                                            const gdl_dice_options* opt, float* sums, float* loss, float* ws, int64_t ws_bytes,
                                            gdl_stream_t stream) {
  return dice_binary_fwd_run(logits, target, total, eps, DiceFamilyOpt(opt), "gdl_dice_binary_loss_fwd", sums, loss, ws, ws_bytes, stream);
}
extern "C" int gdl_dice_binary_loss_fwd(const float* logits, const int64_t* target, int64_t total, float eps,
                                        float* sums, float* loss, float* ws, int64_t ws_bytes, gdl_stream_t stream) {
  return gdl_dice_binary_loss_opt_fwd(logits, target, total, eps, nullptr, sums, loss, ws, ws_bytes, stream);
}
extern "C" int gdl_overlap_binary_loss_fwd(const float* logits, const int64_t* target, int64_t total, float eps,
                                           const gdl_overlap_options* opt, float* sums, float* loss, float* ws, int64_t ws_bytes,
                                           gdl_stream_t stream) {
  return dice_binary_fwd_run(logits, target, total, eps, DiceFamilyOpt(opt), "gdl_overlap_binary_loss_fwd", sums, loss, ws, ws_bytes, stream);
}

static int dice_binary_bwd_run(const float* logits, const int64_t* target, int64_t total, float eps, DiceFamilyOpt opt,
                               const char* who, const float* sums, const float* upstream, float grad_scale, float* dlogits,
                               int accumulate, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && sums && dlogits, "%s: null pointer", who);
  DiceHostOpt h;
  if (const int st = opt.resolve(1, who, h); st != GDL_OK) return st;
  IGN_SWITCH(h.ign, hipLaunchKernelGGL((dice_binary_bwd_kernel<IG>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, logits, target,
                                total, sums, eps, upstream, grad_scale, dlogits, accumulate, h.ignore, h.o));
  GDL_CHECK_LAUNCH(who);
  return GDL_OK;
}
extern "C" int gdl_dice_binary_loss_opt_bwd(const float* logits, const int64_t* target, int64_t total, float eps,
                                            const gdl_dice_options* opt, const float* sums, const float* upstream,
                                            float grad_scale, float* dlogits, int accumulate, gdl_stream_t stream) {
  return dice_binary_bwd_run(logits, target, total, eps, DiceFamilyOpt(opt), "gdl_dice_binary_loss_bwd", sums, upstream, grad_scale, dlogits,
                             accumulate, stream);
}
extern "C" int gdl_dice_binary_loss_bwd(const float* logits, const int64_t* target, int64_t total, float eps,
                                        const float* sums, const float* upstream, float grad_scale, float* dlogits,
                                        int accumulate, gdl_stream_t stream) {
  return gdl_dice_binary_loss_opt_bwd(logits, target, total, eps, nullptr, sums, upstream, grad_scale, dlogits, accumulate, stream);
}
extern "C" int gdl_overlap_binary_loss_bwd(const float* logits, const int64_t* target, int64_t total, float eps,
                                           const gdl_overlap_options* opt, const float* sums, const float* upstream,
                                           float grad_scale, float* dlogits, int accumulate, gdl_stream_t stream) {
  return dice_binary_bwd_run(logits, target, total, eps, DiceFamilyOpt(opt), "gdl_overlap_binary_loss_bwd", sums, upstream, grad_scale, dlogits,
                             accumulate, stream);
}

// ---- binary, from the low-resolution map: low [B, Hi, Wi, 1], target [B, Ho, Wo]; forward workspace: gdl_dice_loss_lowres_workspace(B, 1,
// Ho, Wo).  Shape limits of the multiclass low-resolution entry points: an upsample by at most 64 per direction.
static int dice_binary_lowres_fwd_run(const float* low, const int64_t* target, int B, int Hi, int Wi, int Ho, int Wo, float eps,
                                      DiceFamilyOpt opt, const char* who, float* sums, float* loss, float* ws, int64_t ws_bytes,
                                      gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && sums && loss && ws, "%s: null pointer", who);
  LOWRES_SHAPE(who, 1);
  GDL_CHECK_ARG(ws_bytes >= gdl_dice_loss_lowres_workspace(B, 1, Ho, Wo), "%s: workspace too small", who);
  DiceHostOpt h;
  if (const int st = opt.resolve(1, who, h); st != GDL_OK) return st;
  const int nblk = dice_lowres_blocks((int64_t)B * Ho * Wo);
  hipStream_t s = (hipStream_t)stream;
  IGN_SWITCH(h.ign, hipLaunchKernelGGL((dice_binary_lowres_partial_kernel<IG>), dim3(nblk), dim3(256), 0, s, low, target, B, Hi, Wi, Ho, Wo, ws, h.ignore));
  hipLaunchKernelGGL((dice_final_kernel<1>), dim3(1), dim3(256), 0, s, ws, nblk, eps, sums, loss, h.o);
  GDL_CHECK_LAUNCH(who);
  return GDL_OK;
}
extern "C" int gdl_dice_binary_loss_lowres_opt_fwd(const float* low, const int64_t* target, int B, int Hi, int Wi, int Ho, int Wo,
                                                   float eps, const gdl_dice_options* opt, float* sums, float* loss, float* ws,
                                                   int64_t ws_bytes, gdl_stream_t stream) {
  return dice_binary_lowres_fwd_run(low, target, B, Hi, Wi, Ho, Wo, eps, DiceFamilyOpt(opt), "gdl_dice_binary_loss_lowres_opt_fwd", sums, loss, ws, ws_bytes, stream);
}
extern "C" int gdl_dice_binary_loss_lowres_fwd(const float* low, const int64_t* target, int B, int Hi, int Wi, int Ho, int Wo, float eps,
                                               float* sums, float* loss, float* ws, int64_t ws_bytes, gdl_stream_t stream) {
  return dice_binary_lowres_fwd_run(low, target, B, Hi, Wi, Ho, Wo, eps, DiceFamilyOpt((const gdl_dice_options*)nullptr), "gdl_dice_binary_loss_lowres_fwd", sums, loss, ws, ws_bytes, stream);
}
extern "C" int gdl_overlap_binary_loss_lowres_fwd(const float* low, const int64_t* target, int B, int Hi, int Wi, int Ho, int Wo,
                                                  float eps, const gdl_overlap_options* opt, float* sums, float* loss, float* ws,
                                                  int64_t ws_bytes, gdl_stream_t stream) {
  return dice_binary_lowres_fwd_run(low, target, B, Hi, Wi, Ho, Wo, eps, DiceFamilyOpt(opt), "gdl_overlap_binary_loss_lowres_fwd", sums, loss, ws, ws_bytes, stream);
}

// bytes of scratch the tile form of the binary low-resolution backwards needs (0: the shape takes the gather kernel only)
extern "C" int64_t gdl_binary_lowres_bwd_workspace(int B, int Hi, int Wi, int Ho, int Wo) {
  return lowres_bwd_need(1, true, B, Hi, Wi, Ho, Wo);
}

static int dice_binary_lowres_bwd_run(const float* low, const int64_t* target, int B, int Hi, int Wi, int Ho, int Wo, float eps,
                                      DiceFamilyOpt opt, const char* who, const float* sums, const float* upstream, float grad_scale,
                                      float* dlow, float* ws, int64_t ws_bytes, int form, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && sums && dlow, "%s: null pointer", who);
  LOWRES_SHAPE(who, 1);
  DiceHostOpt h;
  if (const int st = opt.resolve(1, who, h); st != GDL_OK) return st;
  auto a = lowres_args(low, target, B, Hi, Wi, Ho, Wo, upstream, grad_scale, nullptr, dlow, DiceBinaryOpt{sums, eps, h.ignore, h.o});
  IGN_SWITCH(h.ign, return lowres_bwd<DiceBinaryPix<IG>>(who, a, 1, form, ws, ws_bytes, (hipStream_t)stream));
}
extern "C" int gdl_dice_binary_loss_lowres_opt_bwd(const float* low, const int64_t* target, int B, int Hi, int Wi, int Ho, int Wo,
                                                   float eps, const gdl_dice_options* opt, const float* sums, const float* upstream,
                                                   float grad_scale, float* dlow, float* ws, int64_t ws_bytes, int form,
                                                   gdl_stream_t stream) {
  return dice_binary_lowres_bwd_run(low, target, B, Hi, Wi, Ho, Wo, eps, DiceFamilyOpt(opt), "gdl_dice_binary_loss_lowres_opt_bwd", sums, upstream,
                                    grad_scale, dlow, ws, ws_bytes, form, stream);
}
extern "C" int gdl_dice_binary_loss_lowres_bwd(const float* low, const int64_t* target, int B, int Hi, int Wi, int Ho, int Wo, float eps,
                                               const float* sums, const float* upstream, float grad_scale, float* dlow, float* ws,
                                               int64_t ws_bytes, int form, gdl_stream_t stream) {
  return dice_binary_lowres_bwd_run(low, target, B, Hi, Wi, Ho, Wo, eps, DiceFamilyOpt((const gdl_dice_options*)nullptr),
                                    "gdl_dice_binary_loss_lowres_bwd", sums, upstream, grad_scale, dlow, ws, ws_bytes, form, stream);
}
extern "C" int gdl_overlap_binary_loss_lowres_bwd(const float* low, const int64_t* target, int B, int Hi, int Wi, int Ho, int Wo,
                                                  float eps, const gdl_overlap_options* opt, const float* sums, const float* upstream,
                                                  float grad_scale, float* dlow, float* ws, int64_t ws_bytes, int form,
                                                  gdl_stream_t stream) {
  return dice_binary_lowres_bwd_run(low, target, B, Hi, Wi, Ho, Wo, eps, DiceFamilyOpt(opt), "gdl_overlap_binary_loss_lowres_bwd", sums, upstream,
                                    grad_scale, dlow, ws, ws_bytes, form, stream);
}
