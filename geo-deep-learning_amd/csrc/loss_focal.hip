// Focal loss (binary and multiclass): smp 0.5.0 FocalLoss (losses/focal.py, losses/_functional.py::focal_loss_with_logits).
//
// Per element, for logit x and z = [y == k] (multiclass, every class k) or [y == 1] (binary), with s = (2z - 1) x:
//   L  = softplus(-s) = max(-s, 0) + log1p(exp(-|s|))       (BCE with logits, -log pt)
//   q  = sigmoid(-s) = 1 - pt,   pt = sigmoid(s)            (each from e = exp(-|s|): e / (1 + e) or 1 / (1 + e) -- no 1 - x)
//   f  = q^gamma = exp(-gamma softplus(s));  with reduced_threshold th: f = (q / th)^gamma, and f = 1 where pt < th
//   a  = alpha z + (1 - alpha)(1 - z), or 1 without alpha
//   l  = a f L
//   dl/dx = -(2z - 1) a f (gamma pt L + q)                  (-(2z - 1) a q on the f = 1 branch): finite for every gamma >= 0
//   loss  = sum_k sum_valid l / n,  n = the number of valid pixels (y != ignore_index) for "mean", 1 for "sum";  n = 0 -> 0
// A target outside 0..K-1 that is not ignore_index matches no class and stays a valid all-negative pixel: the target is only
// ever compared, never used as an index.  The loss has no cross-class coupling, so every kernel walks the classes one by one.
//
// No float atomics (same input -> same bits on every launch): per-workgroup f64 partials of the loss and of the valid count, one
// workgroup adds them in a fixed order, applies the divisor ON THE DEVICE and leaves it in `norm` for the backward: nothing
// synchronises with the host.
//   full resolution -- NCHW f32 logits, one thread per pixel, the target read once per pixel, every access coalesced over pixels;
//                      any K >= 1.  Binary mode is the same pair of kernels on [1, 1, total] with the class test y == 1.
//   low resolution  -- the head's NHWC map [B, Hi, Wi, K] and a target at [Ho, Wo], the bilinear logit evaluated on the fly
//                      (bilinear_index.h).  The forward is a partial-sum pass; the backward recomputes: the tile form of
//                      lowres_tile.h (K <= 8, every full-resolution element evaluated once) or the gather kernel (K <= 16).
#include "gdl_common.h"
#include "bilinear_index.h"
#include "lowres_tile.h"

namespace {

struct FocalOpt {
  float gamma;
  float a_pos, a_neg;   // the weight of a positive (z = 1) / negative element
  float th;             // reduced_threshold; <= 0: none
  float shift;          // log(th), or 0: f = exp(-gamma (softplus(s) + shift))
  int has_ignore;
  int64_t ignore;
  int64_t cls0;         // the target value of class 0: 0 (multiclass), 1 (binary)
};

__device__ __forceinline__ bool focal_valid(int64_t t, const FocalOpt& o) { return !(o.has_ignore && t == o.ignore); }

// one element: its loss (LOSS) or dl/dx (otherwise), see the top of the file
template <bool LOSS>
__device__ __forceinline__ float focal_elem(float x, bool z, const FocalOpt& o) {
  const float ax = fabsf(x);
  const float e = expf(-ax), lp = log1pf(e), r = 1.f / (1.f + e);
  const bool pos = z ? x >= 0.f : x <= 0.f;                 // s >= 0
  const float L = (pos ? 0.f : ax) + lp;                    // softplus(-s)
  const float sp = (pos ? ax : 0.f) + lp;                   // softplus(s)
  const float q = pos ? e * r : r, pt = pos ? r : e * r;
  const bool flat = o.th > 0.f && pt < o.th;                // the f = 1 branch of reduced_threshold
  float f = o.gamma == 2.f && !(o.th > 0.f) ? q * q : expf(-o.gamma * (sp + o.shift));
  f = flat ? 1.f : f;
  const float a = z ? o.a_pos : o.a_neg;
  if (LOSS) return a * f * L;
  const float g = a * f * ((flat ? 0.f : o.gamma) * pt * L + q);
  return z ? -g : g;
}

// ------------------------------------------------------------------ full resolution (and binary: B = 1, K = 1, cls0 = 1)
// ws[0 .. n) = loss partials, ws[n .. 2n) = valid-pixel counts (exact in f64)
__global__ __launch_bounds__(256) void focal_partial_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B,
                                                            int K, int64_t HW, double* __restrict__ ws, const FocalOpt o) {
  const int64_t total = (int64_t)B * HW;
  double acc = 0.0, cnt = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = target[i];
    if (!focal_valid(t, o)) continue;
    const int64_t b = i / HW, p = i - b * HW;
    const float* px = logits + b * K * HW + p;
    float l = 0.f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) l += focal_elem<true>(px[(int64_t)k * HW], t == (int64_t)k + o.cls0, o);
    acc += (double)l;
    cnt += 1.0;
  }
  block256_store_sum(acc, ws);
  __syncthreads();      // block256_store_sum's LDS slots are reused
  block256_store_sum(cnt, ws + gridDim.x);
}

// one workgroup: the two sums of n partials each in a fixed order (strided per thread, then a tree); the divisor
// (mean: 1 / valid count, 0 without a valid pixel; sum: 1) -> norm[0], loss = sum * divisor
__global__ __launch_bounds__(256) void focal_final_kernel(const double* __restrict__ ws, int n, int mean, float* __restrict__ loss,
                                                          float* __restrict__ norm) {
  __shared__ double part[256], pcnt[256];
  const int t = threadIdx.x;
  double acc = 0.0, cnt = 0.0;
#pragma unroll 8
  for (int i = t; i < n; i += 256) acc += ws[i];
#pragma unroll 8
  for (int i = t; i < n; i += 256) cnt += ws[n + i];
  part[t] = acc;
  pcnt[t] = cnt;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      part[t] += part[t + s];
      pcnt[t] += pcnt[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double inv = mean ? (pcnt[0] > 0.0 ? 1.0 / pcnt[0] : 0.0) : 1.0;
    loss[0] = (float)(part[0] * inv);
    norm[0] = (float)inv;
  }
}

__global__ __launch_bounds__(256) void focal_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B, int K,
                                                        int64_t HW, const float* __restrict__ norm, const float* __restrict__ upstream,
                                                        float scale, float* __restrict__ dlogits, int accumulate, const FocalOpt o) {
  const float c = (upstream ? upstream[0] : 1.f) * scale * norm[0];
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = target[i];
    const bool valid = focal_valid(t, o);
    const int64_t b = i / HW, p = i - b * HW;
    const float* px = logits + b * K * HW + p;
    float* pd = dlogits + b * K * HW + p;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const int64_t at = (int64_t)k * HW;
      const float v = valid ? c * focal_elem<false>(px[at], t == (int64_t)k + o.cls0, o) : 0.f;      // an ignored pixel: exactly zero
      pd[at] = accumulate ? pd[at] + v : v;
    }
  }
}

// ------------------------------------------------------------------ low resolution
// BIN (K = 1 only): the binary loss on the one-class head's map [B, Hi, Wi, 1] -- the class test is y == cls0 (= 1), as the
// full-resolution kernels take it from FocalOpt; without BIN the test is y == k and the multiclass code is what it was.
template <int K, bool BIN = false>
__global__ __launch_bounds__(256) void focal_lowres_partial_kernel(const float* __restrict__ low, const int64_t* __restrict__ target,
                                                                   int B, int Hi, int Wi, int Ho, int Wo, double* __restrict__ ws,
                                                                   const FocalOpt o) {
  const int64_t total = (int64_t)B * Ho * Wo;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  double acc = 0.0, cnt = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = target[i];
    if (!focal_valid(t, o)) continue;
    const int ox = (int)(i % Wo);
    const int64_t r = i / Wo;
    const int oy = (int)(r % Ho), b = (int)(r / Ho);
    int y0, y1, x0, x1; float ly, lx;
    src_index2(ry, oy, Hi, y0, y1, ly);
    src_index2(rx, ox, Wi, x0, x1, lx);
    float x[K], l = 0.f;
    bilinear_logits<K>(low, b, Hi, Wi, y0, y1, x0, x1, ly, lx, x);
#pragma unroll
    for (int k = 0; k < K; ++k) l += focal_elem<true>(x[k], BIN ? t == o.cls0 : t == (int64_t)k, o);
    acc += (double)l;
    cnt += 1.0;
  }
  block256_store_sum(acc, ws);
  __syncthreads();
  block256_store_sum(cnt, ws + gridDim.x);
}

// gather form: one thread per LOW-resolution logit vector sums wy * wx * dl/dlogit over the full-resolution pixels that interpolate
// from it, rows then columns in ascending order.  Every class count up to 16; each full-resolution element is evaluated once per
// low-resolution neighbour (up to four times).
template <int K, bool BIN = false>
__global__ __launch_bounds__(256) void focal_lowres_bwd_gather_kernel(const float* __restrict__ low, const int64_t* __restrict__ target,
                                                                      int B, int Hi, int Wi, int Ho, int Wo,
                                                                      const float* __restrict__ norm, const float* __restrict__ upstream,
                                                                      float scale, float* __restrict__ dlow, const FocalOpt o) {
  const float c = (upstream ? upstream[0] : 1.f) * scale * norm[0];
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
        if (!focal_valid(t, o)) continue;      // an ignored pixel adds nothing
        float x[K];
        bilinear_logits<K>(low, b, Hi, Wi, y0, y1, x0, x1, ly, lx, x);
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += w * focal_elem<false>(x[k], BIN ? t == o.cls0 : t == (int64_t)k, o);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) dlow[i * K + k] = c * acc[k];
  }
}

// tile form (lowres_tile.h): dl/dlogit of the tile's pixels (unscaled) -> LDS, then the shared transposed resize into the tile's
// partial patch; lowres_reduce_kernel applies upstream * scale * norm.  K <= 8.
struct FocalTile : LowresTile {
  FocalOpt o;
};

template <int K, bool BIN = false>
__global__ __launch_bounds__(CT_T) void focal_lowres_tile_kernel(const FocalTile a) {
  extern __shared__ __attribute__((aligned(16))) float csm[];
  float* dl = csm;                                   // [K][CT_H][CT_W]
  const TileAt at = lowres_tile_at(a);
  for (int i = threadIdx.x; i < CT_H * CT_W; i += CT_T) {
    const int r = i / CT_W, c = i - r * CT_W;
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.f;
    if (r < at.rows && c < at.cols) {
      const int oy = at.oy0 + r, ox = at.ox0 + c;
      const int64_t t = a.target[((int64_t)at.b * a.Ho + oy) * a.Wo + ox];
      if (focal_valid(t, a.o)) {
        int y0, y1, x0, x1; float ly, lx;
        src_index2(at.ry, oy, a.Hi, y0, y1, ly);
        src_index2(at.rx, ox, a.Wi, x0, x1, lx);
        float x[K];
        bilinear_logits<K>(a.low, at.b, a.Hi, a.Wi, y0, y1, x0, x1, ly, lx, x);
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = focal_elem<false>(x[k], BIN ? t == a.o.cls0 : t == (int64_t)k, a.o);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) dl[(k * CT_H + r) * CT_W + c] = v[k];
  }
  lowres_tile_patch<K>(a, at, csm, [] {});
}

}  // namespace

// ============================================================================ C ABI
#define FOCAL_OPT_PARAMS float gamma, int has_alpha, float alpha, int has_threshold, float threshold, int has_ignore, int64_t ignore, int mean

static int focal_host_opt(const char* who, int K, FOCAL_OPT_PARAMS, int64_t cls0, FocalOpt& o) {
  (void)mean;
  GDL_CHECK_ARG(K >= 1, "%s: K=%d classes", who, K);
  GDL_CHECK_ARG(gamma >= 0.f && gamma <= 3.0e38f, "%s: gamma %g must be finite and >= 0", who, (double)gamma);
  GDL_CHECK_ARG(!has_alpha || (alpha >= 0.f && alpha <= 1.f), "%s: alpha %g outside [0, 1]", who, (double)alpha);
  GDL_CHECK_ARG(!has_threshold || (threshold > 0.f && threshold <= 1.f), "%s: reduced_threshold %g outside (0, 1]", who, (double)threshold);
  o.gamma = gamma;
  o.a_pos = has_alpha ? alpha : 1.f;
  o.a_neg = has_alpha ? 1.f - alpha : 1.f;
  o.th = has_threshold ? threshold : 0.f;
  o.shift = has_threshold ? logf(threshold) : 0.f;
  o.has_ignore = has_ignore != 0;
  o.ignore = ignore;
  o.cls0 = cls0;
  return GDL_OK;
}
#define FOCAL_OPT(who, K, cls0)                                                                                                          \
  FocalOpt o;                                                                                                                            \
  { const int st_ = focal_host_opt(who, K, gamma, has_alpha, alpha, has_threshold, threshold, has_ignore, ignore, mean, cls0, o);        \
    if (st_ != GDL_OK) return st_; }

// (2048 pixels per workgroup up to 2048 workgroups, as gdl_soft_ce_fwd: a streaming read wants every SIMD full)
static int focal_blocks(int64_t total, int per_block) {
  int64_t g = (total + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

static int focal_fwd(const char* who, const float* logits, const int64_t* target, int B, int K, int64_t HW, int mean, float* loss,
                     float* norm, void* ws, int64_t ws_bytes, gdl_stream_t stream, const FocalOpt& o) {
  GDL_CHECK_ARG(logits && target && loss && norm && ws, "%s: null pointer", who);
  GDL_CHECK_ARG(B > 0 && HW > 0, "%s: bad sizes", who);
  GDL_CHECK_ARG(ws_bytes >= gdl_focal_workspace(B, K, HW) && (uintptr_t)ws % 8 == 0, "%s: workspace too small or misaligned", who);
  const int nblk = focal_blocks((int64_t)B * HW, 2048);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(focal_partial_kernel, dim3(nblk), dim3(256), 0, s, logits, target, B, K, HW, (double*)ws, o);
  hipLaunchKernelGGL(focal_final_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, nblk, mean, loss, norm);
  GDL_CHECK_LAUNCH(who);
  return GDL_OK;
}

static int focal_bwd(const char* who, const float* logits, const int64_t* target, int B, int K, int64_t HW, const float* norm,
                     const float* upstream, float grad_scale, float* dlogits, int accumulate, gdl_stream_t stream, const FocalOpt& o) {
  GDL_CHECK_ARG(logits && target && norm && dlogits, "%s: null pointer", who);
  GDL_CHECK_ARG(B > 0 && HW > 0, "%s: bad sizes", who);
  hipLaunchKernelGGL(focal_bwd_kernel, dim3(grid_for((int64_t)B * HW)), dim3(256), 0, (hipStream_t)stream, logits, target, B, K, HW, norm,
                     upstream, grad_scale, dlogits, accumulate, o);
  GDL_CHECK_LAUNCH(who);
  return GDL_OK;
}

extern "C" int64_t gdl_focal_workspace(int B, int K, int64_t HW) {
  (void)K;
  return 2 * (int64_t)focal_blocks((int64_t)B * HW, 2048) * (int64_t)sizeof(double);
}

extern "C" int gdl_focal_fwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, FOCAL_OPT_PARAMS, float* loss,
                             float* norm, void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  FOCAL_OPT("gdl_focal_fwd", K, 0);
  return focal_fwd("gdl_focal_fwd", logits, target, B, K, HW, mean, loss, norm, ws, ws_bytes, stream, o);
}

extern "C" int gdl_focal_bwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, FOCAL_OPT_PARAMS, const float* norm,
                             const float* upstream, float grad_scale, float* dlogits, int accumulate, gdl_stream_t stream) {
  FOCAL_OPT("gdl_focal_bwd", K, 0);
  return focal_bwd("gdl_focal_bwd", logits, target, B, K, HW, norm, upstream, grad_scale, dlogits, accumulate, stream, o);
}

// ---- binary: z = [y == 1] on `total` logits (workspace: gdl_focal_workspace(1, 1, total))
extern "C" int gdl_focal_binary_fwd(const float* logits, const int64_t* target, int64_t total, FOCAL_OPT_PARAMS, float* loss, float* norm,
                                    void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  FOCAL_OPT("gdl_focal_binary_fwd", 1, 1);
  return focal_fwd("gdl_focal_binary_fwd", logits, target, 1, 1, total, mean, loss, norm, ws, ws_bytes, stream, o);
}

extern "C" int gdl_focal_binary_bwd(const float* logits, const int64_t* target, int64_t total, FOCAL_OPT_PARAMS, const float* norm,
                                    const float* upstream, float grad_scale, float* dlogits, int accumulate, gdl_stream_t stream) {
  FOCAL_OPT("gdl_focal_binary_bwd", 1, 1);
  return focal_bwd("gdl_focal_binary_bwd", logits, target, 1, 1, total, norm, upstream, grad_scale, dlogits, accumulate, stream, o);
}

// ---- low resolution
#define FOCAL_LOWRES_SHAPE(who)                                                                                                   \
  GDL_CHECK_ARG(B > 0 && Hi > 0 && Wi > 0 && Ho >= Hi && Wo >= Wi, who ": bad sizes (an upsample is expected)");                  \
  GDL_CHECK_ARG((Ho + Hi - 1) / Hi <= LOWRES_MAX_FACTOR && (Wo + Wi - 1) / Wi <= LOWRES_MAX_FACTOR,                               \
                who ": upsampling factors above 64 are not supported");                                                           \
  GDL_CHECK_ARG(K >= 1 && K <= 16, who ": K=%d classes unsupported (1..16)", K)

// (1024 pixels per workgroup, as the Dice and soft-CE low-resolution forwards: the scattered loads are latency bound)
extern "C" int64_t gdl_focal_lowres_workspace(int B, int K, int Ho, int Wo) {
  (void)K;
  return 2 * (int64_t)focal_blocks((int64_t)B * Ho * Wo, 1024) * (int64_t)sizeof(double);
}

extern "C" int gdl_focal_lowres_fwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo,
                                    FOCAL_OPT_PARAMS, float* loss, float* norm, void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && loss && norm && ws, "gdl_focal_lowres_fwd: null pointer");
  FOCAL_LOWRES_SHAPE("gdl_focal_lowres_fwd");
  GDL_CHECK_ARG(ws_bytes >= gdl_focal_lowres_workspace(B, K, Ho, Wo) && (uintptr_t)ws % 8 == 0,
                "gdl_focal_lowres_fwd: workspace too small or misaligned");
  FOCAL_OPT("gdl_focal_lowres_fwd", K, 0);
  const int nblk = focal_blocks((int64_t)B * Ho * Wo, 1024);
  hipStream_t s = (hipStream_t)stream;
  K_SWITCH(K, hipLaunchKernelGGL((focal_lowres_partial_kernel<KK>), dim3(nblk), dim3(256), 0, s, low, target, B, Hi, Wi, Ho, Wo, (double*)ws, o));
  hipLaunchKernelGGL(focal_final_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, nblk, mean, loss, norm);
  GDL_CHECK_LAUNCH("gdl_focal_lowres_fwd");
  return GDL_OK;
}

// bytes of scratch the tile form of gdl_focal_lowres_bwd needs (0: the shape takes the gather kernel only)
extern "C" int64_t gdl_focal_lowres_bwd_workspace(int B, int K, int Hi, int Wi, int Ho, int Wo) {
  int ny, nx;
  if (B <= 0 || K < 1 || Hi <= 0 || Wi <= 0 || Ho < Hi || Wo < Wi || !lowres_tile_dims(K, Hi, Wi, Ho, Wo, ny, nx)) return 0;
  return lowres_tiles(B, Ho, Wo) * ny * nx * K * (int64_t)sizeof(float);
}

extern "C" int gdl_focal_lowres_bwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo, FOCAL_OPT_PARAMS,
                                    const float* norm, const float* upstream, float grad_scale, float* dlow, float* ws, int64_t ws_bytes,
                                    int form, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && norm && dlow, "gdl_focal_lowres_bwd: null pointer");
  FOCAL_LOWRES_SHAPE("gdl_focal_lowres_bwd");
  GDL_CHECK_ARG(form == GDL_FOCAL_AUTO || form == GDL_FOCAL_GATHER || form == GDL_FOCAL_TILE, "gdl_focal_lowres_bwd: unknown form %d", form);
  FOCAL_OPT("gdl_focal_lowres_bwd", K, 0);
  hipStream_t st = (hipStream_t)stream;
  int ny, nx;
  const int64_t need = gdl_focal_lowres_bwd_workspace(B, K, Hi, Wi, Ho, Wo);
  const bool can_tile = need > 0 && ws && ws_bytes >= need && lowres_tile_dims(K, Hi, Wi, Ho, Wo, ny, nx);
  GDL_CHECK_ARG(form != GDL_FOCAL_TILE || can_tile, "gdl_focal_lowres_bwd: this shape or workspace does not take the tile form");
  if (can_tile && form != GDL_FOCAL_GATHER) {
    FocalTile a{};
    a.low = low; a.target = target; a.upstream = upstream; a.patches = ws; a.dlow = dlow; a.norm = norm;
    lowres_tile_shape(a, B, Hi, Wi, Ho, Wo, ny, nx);
    a.scale = grad_scale; a.o = o;
    const unsigned tiles = (unsigned)lowres_tiles(B, Ho, Wo);
    K_SWITCH(K, if (KK <= 8) {
                     constexpr int K8 = KK <= 8 ? KK : 8;
                     GDL_SET_MAX_LDS_ONCE((focal_lowres_tile_kernel<K8>), 159 * 1024);
                     hipLaunchKernelGGL((focal_lowres_tile_kernel<K8>), dim3(tiles), dim3(CT_T), lowres_tile_lds(K8, ny, nx), st, a);
                   });
    const int rc = lowres_launch_reduce(a, K, st);
    if (rc != GDL_OK) return rc;
    GDL_CHECK_LAUNCH("gdl_focal_lowres_bwd");
    return GDL_OK;
  }
  const int64_t total = (int64_t)B * Hi * Wi;
  K_SWITCH(K, hipLaunchKernelGGL((focal_lowres_bwd_gather_kernel<KK>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, low, target, B,
                                    Hi, Wi, Ho, Wo, norm, upstream, grad_scale, dlow, o));
  GDL_CHECK_LAUNCH("gdl_focal_lowres_bwd");
  return GDL_OK;
}

// ---- binary, from the low-resolution map: low [B, Hi, Wi, 1], target [B, Ho, Wo], z = [y == 1]; the kernels above at K = 1 with
// the class test of FocalOpt::cls0.  Workspaces: gdl_focal_lowres_workspace(B, 1, Ho, Wo), gdl_binary_lowres_bwd_workspace().
extern "C" int gdl_focal_binary_lowres_fwd(const float* low, const int64_t* target, int B, int Hi, int Wi, int Ho, int Wo,
                                           FOCAL_OPT_PARAMS, float* loss, float* norm, void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  const int K = 1;
  GDL_CHECK_ARG(low && target && loss && norm && ws, "gdl_focal_binary_lowres_fwd: null pointer");
  FOCAL_LOWRES_SHAPE("gdl_focal_binary_lowres_fwd");
  GDL_CHECK_ARG(ws_bytes >= gdl_focal_lowres_workspace(B, K, Ho, Wo) && (uintptr_t)ws % 8 == 0,
                "gdl_focal_binary_lowres_fwd: workspace too small or misaligned");
  FOCAL_OPT("gdl_focal_binary_lowres_fwd", K, 1);
  const int nblk = focal_blocks((int64_t)B * Ho * Wo, 1024);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL((focal_lowres_partial_kernel<1, true>), dim3(nblk), dim3(256), 0, s, low, target, B, Hi, Wi, Ho, Wo, (double*)ws, o);
  hipLaunchKernelGGL(focal_final_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, nblk, mean, loss, norm);
  GDL_CHECK_LAUNCH("gdl_focal_binary_lowres_fwd");
  return GDL_OK;
}

extern "C" int gdl_focal_binary_lowres_bwd(const float* low, const int64_t* target, int B, int Hi, int Wi, int Ho, int Wo,
                                           FOCAL_OPT_PARAMS, const float* norm, const float* upstream, float grad_scale, float* dlow,
                                           float* ws, int64_t ws_bytes, int form, gdl_stream_t stream) {
  const int K = 1;
  GDL_CHECK_ARG(low && target && norm && dlow, "gdl_focal_binary_lowres_bwd: null pointer");
  FOCAL_LOWRES_SHAPE("gdl_focal_binary_lowres_bwd");
  GDL_CHECK_ARG(form == GDL_FOCAL_AUTO || form == GDL_FOCAL_GATHER || form == GDL_FOCAL_TILE, "gdl_focal_binary_lowres_bwd: unknown form %d", form);
  FOCAL_OPT("gdl_focal_binary_lowres_bwd", K, 1);
  hipStream_t st = (hipStream_t)stream;
  int ny, nx;
  const int64_t need = gdl_binary_lowres_bwd_workspace(B, Hi, Wi, Ho, Wo);
  const bool can_tile = need > 0 && ws && ws_bytes >= need && binary_tile_dims(Hi, Wi, Ho, Wo, ny, nx);
  GDL_CHECK_ARG(form != GDL_FOCAL_TILE || can_tile, "gdl_focal_binary_lowres_bwd: this shape or workspace does not take the tile form");
  if (can_tile && form != GDL_FOCAL_GATHER) {
    FocalTile a{};
    a.low = low; a.target = target; a.upstream = upstream; a.patches = ws; a.dlow = dlow; a.norm = norm;
    lowres_tile_shape(a, B, Hi, Wi, Ho, Wo, ny, nx);
    a.scale = grad_scale; a.o = o;
    hipLaunchKernelGGL((focal_lowres_tile_kernel<1, true>), dim3((unsigned)lowres_tiles(B, Ho, Wo)), dim3(CT_T), lowres_tile_lds(1, ny, nx), st, a);
    const int rc = lowres_launch_reduce(a, K, st);
    if (rc != GDL_OK) return rc;
    GDL_CHECK_LAUNCH("gdl_focal_binary_lowres_bwd");
    return GDL_OK;
  }
  const int64_t total = (int64_t)B * Hi * Wi;
  hipLaunchKernelGGL((focal_lowres_bwd_gather_kernel<1, true>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, low, target, B, Hi, Wi,
                     Ho, Wo, norm, upstream, grad_scale, dlow, o);
  GDL_CHECK_LAUNCH("gdl_focal_binary_lowres_bwd");
  return GDL_OK;
}
