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
//                      (bilinear_index.h).  The forward is a partial-sum pass; the backward recomputes: the tile form
//                      (K <= 8, every full-resolution element evaluated once) or the gather form (K <= 16).  The kernels are
//                      the skeletons of lowres_tile.h with the policy FocalPix.
#include "gdl_common.h"
#include "bilinear_index.h"
#include "lowres_tile.h"
#include "mean_final.h"

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

// ------------------------------------------------------------------ low resolution: the policy of lowres_tile.h
// BIN: the binary loss on the one-class head's map [B, Hi, Wi, 1] -- the class test is y == cls0 (= 1), as the full-resolution
// kernels take it from FocalOpt; without BIN the test is y == k.
template <bool BIN>
struct FocalPix {
  typedef FocalOpt Opt;
  typedef int64_t Target;
  static constexpr bool ONE_CLASS = BIN, COUNTS = true;
  FocalOpt o;
  __device__ FocalPix(const FocalOpt& opt, int) : o(opt) {}
  __device__ bool valid(int64_t t) const { return focal_valid(t, o); }
  __device__ float count(int64_t) const { return 1.f; }
  template <int K>
  __device__ void grad(const float (&x)[K], int64_t t, float (&g)[K]) const {
#pragma unroll
    for (int k = 0; k < K; ++k) g[k] = focal_elem<false>(x[k], BIN ? t == o.cls0 : t == (int64_t)k, o);
  }
  template <int K>
  __device__ float loss(const float (&x)[K], int64_t t) const {
    float l = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) l += focal_elem<true>(x[k], BIN ? t == o.cls0 : t == (int64_t)k, o);
    return l;
  }
};

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
#define FOCAL_OPT_ARGS gamma, has_alpha, alpha, has_threshold, threshold, has_ignore, ignore, mean
#define FOCAL_OPT(who, K, cls0)                                                                                                          \
  FocalOpt o;                                                                                                                            \
  { const int st_ = focal_host_opt(who, K, FOCAL_OPT_ARGS, cls0, o);                                                                     \
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
  hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, nblk, mean, loss, norm);
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

// ---- low resolution (forward workspace: 1024 pixels per workgroup, a loss partial and a count each)
extern "C" int64_t gdl_focal_lowres_workspace(int B, int K, int Ho, int Wo) {
  (void)K;
  return 2 * (int64_t)lowres_fwd_blocks((int64_t)B * Ho * Wo) * (int64_t)sizeof(double);
}

template <bool BIN>
static int focal_lowres_fwd(const char* who, const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo,
                            FOCAL_OPT_PARAMS, float* loss, float* norm, void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && loss && norm && ws, "%s: null pointer", who);
  LOWRES_SHAPE(who, K);
  GDL_CHECK_ARG(ws_bytes >= gdl_focal_lowres_workspace(B, K, Ho, Wo) && (uintptr_t)ws % 8 == 0, "%s: workspace too small or misaligned", who);
  FOCAL_OPT(who, K, BIN ? 1 : 0);
  hipStream_t s = (hipStream_t)stream;
  int nblk;
  const int rc = lowres_launch_partial<FocalPix<BIN>>(low, target, B, K, Hi, Wi, Ho, Wo, (double*)ws, o, nblk, s);
  if (rc != GDL_OK) return rc;
  hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, nblk, mean, loss, norm);
  GDL_CHECK_LAUNCH(who);
  return GDL_OK;
}

template <bool BIN>
static int focal_lowres_bwd(const char* who, const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo,
                            FOCAL_OPT_PARAMS, const float* norm, const float* upstream, float grad_scale, float* dlow, float* ws,
                            int64_t ws_bytes, int form, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && norm && dlow, "%s: null pointer", who);
  LOWRES_SHAPE(who, K);
  FOCAL_OPT(who, K, BIN ? 1 : 0);
  auto a = lowres_args(low, target, B, Hi, Wi, Ho, Wo, upstream, grad_scale, norm, dlow, o);
  return lowres_bwd<FocalPix<BIN>>(who, a, K, form, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int gdl_focal_lowres_fwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo,
                                    FOCAL_OPT_PARAMS, float* loss, float* norm, void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  return focal_lowres_fwd<false>("gdl_focal_lowres_fwd", low, target, B, K, Hi, Wi, Ho, Wo, FOCAL_OPT_ARGS, loss, norm, ws, ws_bytes, stream);
}

// bytes of scratch the tile form of gdl_focal_lowres_bwd needs (0: the shape takes the gather kernel only)
extern "C" int64_t gdl_focal_lowres_bwd_workspace(int B, int K, int Hi, int Wi, int Ho, int Wo) {
  return lowres_bwd_need(K, false, B, Hi, Wi, Ho, Wo);
}

extern "C" int gdl_focal_lowres_bwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo, FOCAL_OPT_PARAMS,
                                    const float* norm, const float* upstream, float grad_scale, float* dlow, float* ws, int64_t ws_bytes,
                                    int form, gdl_stream_t stream) {
  return focal_lowres_bwd<false>("gdl_focal_lowres_bwd", low, target, B, K, Hi, Wi, Ho, Wo, FOCAL_OPT_ARGS, norm, upstream, grad_scale, dlow,
                                 ws, ws_bytes, form, stream);
}

// ---- binary, from the low-resolution map: low [B, Hi, Wi, 1], target [B, Ho, Wo], z = [y == 1].  Workspaces:
// gdl_focal_lowres_workspace(B, 1, Ho, Wo), gdl_binary_lowres_bwd_workspace().
extern "C" int gdl_focal_binary_lowres_fwd(const float* low, const int64_t* target, int B, int Hi, int Wi, int Ho, int Wo,
                                           FOCAL_OPT_PARAMS, float* loss, float* norm, void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  return focal_lowres_fwd<true>("gdl_focal_binary_lowres_fwd", low, target, B, 1, Hi, Wi, Ho, Wo, FOCAL_OPT_ARGS, loss, norm, ws, ws_bytes, stream);
}

extern "C" int gdl_focal_binary_lowres_bwd(const float* low, const int64_t* target, int B, int Hi, int Wi, int Ho, int Wo,
                                           FOCAL_OPT_PARAMS, const float* norm, const float* upstream, float grad_scale, float* dlow,
                                           float* ws, int64_t ws_bytes, int form, gdl_stream_t stream) {
  return focal_lowres_bwd<true>("gdl_focal_binary_lowres_bwd", low, target, B, 1, Hi, Wi, Ho, Wo, FOCAL_OPT_ARGS, norm, upstream, grad_scale,
                                dlow, ws, ws_bytes, form, stream);
}
