// Cross-entropy with class weights and label smoothing: torch.nn.CrossEntropyLoss(weight, ignore_index, reduction, label_smoothing)
// on class-index targets, the loss the reference's own tests train with (tests/test_notebooks_00quickstart.py:63).
//
// With e = label_smoothing, K classes, w_k = weight[k] (all 1 without weights), W = sum_k w_k,
// valid_i = [0 <= y_i < K] * [y_i != ignore_index] and lse_i = logsumexp_k x_ik, per valid pixel:
//   L_i        = (1 - e) w_{y_i} (lse_i - x_{i,y_i}) + (e / K) sum_k w_k (lse_i - x_ik)
//              = (1 - e) w_{y_i} (ls_i - d_{i,y_i}) + (e / K) (W ls_i - sum_k w_k d_ik),   d_ik = x_ik - max_k x_ik <= 0,
//                ls_i = log(sum_k exp(d_ik)) >= 0   (the form evaluated: every term is small and of one sign)
//   dL_i/dx_ik = softmax_k(x_i) ((1 - e) w_{y_i} + (e / K) W) - (1 - e) w_{y_i} [k == y_i] - (e / K) w_k
//   D          = sum_{valid i} w_{y_i};   loss = sum_i L_i / D ("mean"; D = 0 -> loss 0 and gradient 0, where torch gives NaN) or sum_i L_i
// A zero-weight class adds nothing to D or to the first term; its pixels still carry the smoothing term.  A target outside 0..K-1
// that is not ignore_index is treated as ignored (torch device-asserts): the target is only ever compared, never used as an index.
//
// No float atomics (same input -> same bits on every launch): per-workgroup f64 partials of sum L_i and of D, one workgroup adds
// them in a fixed order, applies the divisor ON THE DEVICE and leaves 1 / D in `norm` for the backward (mean_final_kernel): nothing
// synchronises with the host.  The weights are read through their device pointer; a null pointer costs no load.
//   full resolution -- NCHW f32 logits, one thread per pixel, every access coalesced over pixels.  K <= 16 is unrolled over
//                      registers, the weights loaded once per thread; more classes walk the class dimension in a run-time loop
//                      and read the weights from global memory (they stay in L1 / L2).
//   low resolution  -- the head's NHWC map [B, Hi, Wi, K] and a target at [Ho, Wo], the bilinear logit evaluated on the fly
//                      (bilinear_index.h).  The forward is a partial-sum pass; the backward recomputes: the tile form (K <= 8) or
//                      the gather form (K <= 16).  The kernels are the skeletons of lowres_tile.h with the policy XentPix.
#include "gdl_common.h"
#include "bilinear_index.h"
#include "lowres_tile.h"
#include "mean_final.h"

namespace {

struct XentOpt {
  float keep;            // 1 - label_smoothing
  float uni;             // label_smoothing / K
  int has_ignore;
  int64_t ignore;
  const float* weight;   // K class weights on the device; null: all ones
};

__device__ __forceinline__ bool xent_valid(int64_t t, int K, const XentOpt& o) {
  return (uint64_t)t < (uint64_t)K && !(o.has_ignore && t == o.ignore);
}

// the K <= 16 class weights of a thread -> w (registers: only ever indexed by unrolled constants); returns their sum W
__device__ __forceinline__ float xent_weights(const XentOpt& o, int K, float (&w)[16]) {
  float W = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    w[k] = 1.f;
    if (k < K) {
      if (o.weight) w[k] = o.weight[k];
      W += w[k];
    }
  }
  return W;
}

// x[k] -> exp(x[k] - max); returns sum_k of them and the target's weight in wy.  With WITH_LOSS: the pixel's loss in L (see the top
// of the file).  y matches no class for a pixel that is not valid: wy = 0.
template <int K, bool WITH_LOSS>
__device__ __forceinline__ float xent_softmax(float (&x)[K], int y, const float (&w)[16], float W, const XentOpt& o, float& wy, float& L) {
  float mx = x[0];
#pragma unroll
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, x[k]);
  float s = 0.f, swd = 0.f, dy = 0.f;
  wy = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float d = x[k] - mx;
    swd += w[k] * d;
    dy = k == y ? d : dy;
    wy = k == y ? w[k] : wy;
    x[k] = expf(d);
    s += x[k];
  }
  if (WITH_LOSS) {
    const float ls = logf(s);
    L = o.keep * wy * (ls - dy) + o.uni * (W * ls - swd);
  }
  return s;
}

// exp(x[k] - max) in x and the sum s of them -> dL/dlogit in g
template <int K>
__device__ __forceinline__ void xent_grad(const float (&x)[K], float s, int y, float wy, const float (&w)[16], float W, const XentOpt& o,
                                          float (&g)[K]) {
  const float hit = o.keep * wy, a = (hit + o.uni * W) / s;
#pragma unroll
  for (int k = 0; k < K; ++k) g[k] = x[k] * a - (k == y ? hit : 0.f) - o.uni * w[k];
}

// ------------------------------------------------------------------ full resolution
// ws[0 .. n) = loss partials, ws[n .. 2n) = partials of D (the weights of the valid pixels' classes)
template <int K>
__global__ __launch_bounds__(256) void xent_partial_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B,
                                                           int64_t HW, double* __restrict__ ws, const XentOpt o) {
  float w[16];
  const float W = xent_weights(o, K, w);
  const int64_t total = (int64_t)B * HW;
  double acc = 0.0, den = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = target[i];
    if (!xent_valid(t, K, o)) continue;
    const int64_t b = i / HW, p = i - b * HW;
    float x[K], wy, L;
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = logits[(b * K + k) * HW + p];
    xent_softmax<K, true>(x, (int)t, w, W, o, wy, L);
    acc += (double)L;
    den += (double)wy;
  }
  block256_store_sum(acc, ws);
  __syncthreads();      // block256_store_sum's LDS slots are reused
  block256_store_sum(den, ws + gridDim.x);
}

__device__ __forceinline__ float xent_weight_at(const XentOpt& o, int k) { return o.weight ? o.weight[k] : 1.f; }
__device__ __forceinline__ float xent_weight_sum(const XentOpt& o, int K) {
  if (!o.weight) return (float)K;
  float W = 0.f;
  for (int k = 0; k < K; ++k) W += o.weight[k];
  return W;
}

// any class count: the class dimension in two run-time passes (maximum; sums), the second one out of L1 / L2
__global__ __launch_bounds__(256) void xent_partial_any_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B,
                                                               int K, int64_t HW, double* __restrict__ ws, const XentOpt o) {
  const float W = xent_weight_sum(o, K);
  const int64_t total = (int64_t)B * HW;
  double acc = 0.0, den = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = target[i];
    if (!xent_valid(t, K, o)) continue;
    const int64_t b = i / HW, p = i - b * HW;
    const float* px = logits + b * K * HW + p;
    float mx = px[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, px[(int64_t)k * HW]);
    float s = 0.f, swd = 0.f, dy = 0.f, wy = 0.f;
    for (int k = 0; k < K; ++k) {
      const float d = px[(int64_t)k * HW] - mx, wk = xent_weight_at(o, k);
      swd += wk * d;
      dy = (int64_t)k == t ? d : dy;
      wy = (int64_t)k == t ? wk : wy;
      s += expf(d);
    }
    const float ls = logf(s);
    acc += (double)(o.keep * wy * (ls - dy) + o.uni * (W * ls - swd));
    den += (double)wy;
  }
  block256_store_sum(acc, ws);
  __syncthreads();
  block256_store_sum(den, ws + gridDim.x);
}

template <int K>
__global__ __launch_bounds__(256) void xent_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B,
                                                       int64_t HW, const float* __restrict__ norm, const float* __restrict__ upstream,
                                                       float scale, float* __restrict__ dlogits, int accumulate, const XentOpt o) {
  float w[16];
  const float W = xent_weights(o, K, w);
  const float c = (upstream ? upstream[0] : 1.f) * scale * norm[0];
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW, p = i - b * HW;
    const int64_t t = target[i];
    float g[K];
    if (xent_valid(t, K, o)) {
      float x[K], wy, L;
#pragma unroll
      for (int k = 0; k < K; ++k) x[k] = logits[(b * K + k) * HW + p];
      const float s = xent_softmax<K, false>(x, (int)t, w, W, o, wy, L);
      xent_grad<K>(x, s, (int)t, wy, w, W, o, g);
#pragma unroll
      for (int k = 0; k < K; ++k) g[k] *= c;
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) g[k] = 0.f;      // an ignored pixel: exactly zero, whatever its logits and the scalars hold
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int64_t at = (b * K + k) * HW + p;
      dlogits[at] = accumulate ? dlogits[at] + g[k] : g[k];
    }
  }
}

__global__ __launch_bounds__(256) void xent_bwd_any_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B,
                                                           int K, int64_t HW, const float* __restrict__ norm,
                                                           const float* __restrict__ upstream, float scale, float* __restrict__ dlogits,
                                                           int accumulate, const XentOpt o) {
  const float W = xent_weight_sum(o, K);
  const float c = (upstream ? upstream[0] : 1.f) * scale * norm[0];
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW, p = i - b * HW;
    const int64_t t = target[i];
    const float* px = logits + b * K * HW + p;
    float* pd = dlogits + b * K * HW + p;
    if (!xent_valid(t, K, o)) {
      for (int k = 0; k < K; ++k) pd[(int64_t)k * HW] = accumulate ? pd[(int64_t)k * HW] + 0.f : 0.f;
      continue;
    }
    float mx = px[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, px[(int64_t)k * HW]);
    float s = 0.f, wy = 0.f;
    for (int k = 0; k < K; ++k) {
      s += expf(px[(int64_t)k * HW] - mx);
      wy = (int64_t)k == t ? xent_weight_at(o, k) : wy;
    }
    const float hit = o.keep * wy, a = (hit + o.uni * W) / s;
    for (int k = 0; k < K; ++k) {
      const float v = c * (expf(px[(int64_t)k * HW] - mx) * a - ((int64_t)k == t ? hit : 0.f) - o.uni * xent_weight_at(o, k));
      pd[(int64_t)k * HW] = accumulate ? pd[(int64_t)k * HW] + v : v;
    }
  }
}

// ------------------------------------------------------------------ low resolution: the policy of lowres_tile.h
struct XentPix {
  typedef XentOpt Opt;
  typedef int64_t Target;
  static constexpr bool ONE_CLASS = false, COUNTS = true;
  XentOpt o;
  int K;
  float w[16], W;      // the class weights, loaded once per thread, and their sum
  __device__ XentPix(const XentOpt& opt, int classes) : o(opt), K(classes) { W = xent_weights(o, K, w); }
  __device__ bool valid(int64_t t) const { return xent_valid(t, K, o); }
  // the divisor's term of a valid pixel: its class's weight
  __device__ float count(int64_t t) const {
    float wy = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) wy = (k < K && t == (int64_t)k) ? w[k] : wy;
    return wy;
  }
  template <int KK>
  __device__ void grad(float (&x)[KK], int64_t t, float (&g)[KK]) const {
    float wy, L;
    const float s = xent_softmax<KK, false>(x, (int)t, w, W, o, wy, L);
    xent_grad<KK>(x, s, (int)t, wy, w, W, o, g);
  }
  template <int KK>
  __device__ float loss(float (&x)[KK], int64_t t) const {
    float wy, L;
    xent_softmax<KK, true>(x, (int)t, w, W, o, wy, L);
    return L;
  }
};

}  // namespace

// ============================================================================ C ABI
#define XENT_OPT_PARAMS const float* weight, float smooth, int has_ignore, int64_t ignore, int mean
#define XENT_OPT_ARGS weight, smooth, has_ignore, ignore, mean

static int xent_host_opt(const char* who, int K, XENT_OPT_PARAMS, XentOpt& o) {
  (void)mean;
  GDL_CHECK_ARG(K >= 1, "%s: K=%d classes", who, K);
  GDL_CHECK_ARG(smooth >= 0.f && smooth <= 1.f, "%s: label_smoothing %g outside [0, 1]", who, (double)smooth);
  o.keep = 1.f - smooth;
  o.uni = smooth / (float)K;
  o.has_ignore = has_ignore != 0;
  o.ignore = ignore;
  o.weight = weight;
  return GDL_OK;
}
#define XENT_OPT(who, K)                                                                            \
  XentOpt o;                                                                                        \
  { const int st_ = xent_host_opt(who, K, XENT_OPT_ARGS, o); if (st_ != GDL_OK) return st_; }

// (2048 pixels per workgroup up to 2048 workgroups, as gdl_soft_ce_fwd: a streaming read wants every SIMD full)
static int xent_blocks(int64_t total) {
  int64_t g = (total + 2047) / 2048;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

extern "C" int64_t gdl_cross_entropy_workspace(int B, int K, int64_t HW) {
  (void)K;
  return 2 * (int64_t)xent_blocks((int64_t)B * HW) * (int64_t)sizeof(double);
}

extern "C" int gdl_cross_entropy_fwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, XENT_OPT_PARAMS, float* loss,
                                     float* norm, void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && loss && norm && ws, "gdl_cross_entropy_fwd: null pointer");
  GDL_CHECK_ARG(B > 0 && HW > 0, "gdl_cross_entropy_fwd: bad sizes");
  XENT_OPT("gdl_cross_entropy_fwd", K);
  GDL_CHECK_ARG(ws_bytes >= gdl_cross_entropy_workspace(B, K, HW) && (uintptr_t)ws % 8 == 0,
                "gdl_cross_entropy_fwd: workspace too small or misaligned");
  const int nblk = xent_blocks((int64_t)B * HW);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws;
  if (K > 16) {
    hipLaunchKernelGGL(xent_partial_any_kernel, dim3(nblk), dim3(256), 0, s, logits, target, B, K, HW, part, o);
  } else {
    K_SWITCH(K, hipLaunchKernelGGL((xent_partial_kernel<KK>), dim3(nblk), dim3(256), 0, s, logits, target, B, HW, part, o));
  }
  hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, nblk, mean, loss, norm);
  GDL_CHECK_LAUNCH("gdl_cross_entropy_fwd");
  return GDL_OK;
}

extern "C" int gdl_cross_entropy_bwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, XENT_OPT_PARAMS,
                                     const float* norm, const float* upstream, float grad_scale, float* dlogits, int accumulate,
                                     gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && norm && dlogits, "gdl_cross_entropy_bwd: null pointer");
  GDL_CHECK_ARG(B > 0 && HW > 0, "gdl_cross_entropy_bwd: bad sizes");
  XENT_OPT("gdl_cross_entropy_bwd", K);
  const int64_t total = (int64_t)B * HW;
  hipStream_t s = (hipStream_t)stream;
  if (K > 16) {
    hipLaunchKernelGGL(xent_bwd_any_kernel, dim3(grid_for(total)), dim3(256), 0, s, logits, target, B, K, HW, norm, upstream, grad_scale,
                       dlogits, accumulate, o);
  } else {
    K_SWITCH(K, hipLaunchKernelGGL((xent_bwd_kernel<KK>), dim3(grid_for(total)), dim3(256), 0, s, logits, target, B, HW, norm, upstream,
                                   grad_scale, dlogits, accumulate, o));
  }
  GDL_CHECK_LAUNCH("gdl_cross_entropy_bwd");
  return GDL_OK;
}

// ---- low resolution (forward workspace: 1024 pixels per workgroup, a loss partial and a partial of D each)
extern "C" int64_t gdl_cross_entropy_lowres_workspace(int B, int K, int Ho, int Wo) {
  (void)K;
  return 2 * (int64_t)lowres_fwd_blocks((int64_t)B * Ho * Wo) * (int64_t)sizeof(double);
}

extern "C" int gdl_cross_entropy_lowres_fwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo,
                                            XENT_OPT_PARAMS, float* loss, float* norm, void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && loss && norm && ws, "gdl_cross_entropy_lowres_fwd: null pointer");
  LOWRES_SHAPE("gdl_cross_entropy_lowres_fwd", K);
  GDL_CHECK_ARG(ws_bytes >= gdl_cross_entropy_lowres_workspace(B, K, Ho, Wo) && (uintptr_t)ws % 8 == 0,
                "gdl_cross_entropy_lowres_fwd: workspace too small or misaligned");
  XENT_OPT("gdl_cross_entropy_lowres_fwd", K);
  hipStream_t s = (hipStream_t)stream;
  int nblk;
  const int rc = lowres_launch_partial<XentPix>(low, target, B, K, Hi, Wi, Ho, Wo, (double*)ws, o, nblk, s);
  if (rc != GDL_OK) return rc;
  hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, nblk, mean, loss, norm);
  GDL_CHECK_LAUNCH("gdl_cross_entropy_lowres_fwd");
  return GDL_OK;
}

// bytes of scratch the tile form of gdl_cross_entropy_lowres_bwd needs (0: the shape takes the gather kernel only)
extern "C" int64_t gdl_cross_entropy_lowres_bwd_workspace(int B, int K, int Hi, int Wi, int Ho, int Wo) {
  return lowres_bwd_need(K, false, B, Hi, Wi, Ho, Wo);
}

extern "C" int gdl_cross_entropy_lowres_bwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo,
                                            XENT_OPT_PARAMS, const float* norm, const float* upstream, float grad_scale, float* dlow,
                                            float* ws, int64_t ws_bytes, int form, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && norm && dlow, "gdl_cross_entropy_lowres_bwd: null pointer");
  LOWRES_SHAPE("gdl_cross_entropy_lowres_bwd", K);
  XENT_OPT("gdl_cross_entropy_lowres_bwd", K);
  auto a = lowres_args(low, target, B, Hi, Wi, Ho, Wo, upstream, grad_scale, norm, dlow, o);
  return lowres_bwd<XentPix>("gdl_cross_entropy_lowres_bwd", a, K, form, ws, ws_bytes, (hipStream_t)stream);
}
