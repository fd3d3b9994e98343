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
//                       in the backward.  The kernels are the skeletons of lowres_tile.h with the policy CePix.
#include <atomic>

#include "gdl_common.h"
#include "bilinear_index.h"
#include "lowres_tile.h"

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

// ------------------------------------------------------------------ low resolution: the policy of lowres_tile.h
struct CePix {
  typedef CeOpt Opt;
  typedef int64_t Target;
  static constexpr bool ONE_CLASS = false, COUNTS = false;
  CeOpt o;
  int K;
  __device__ CePix(const CeOpt& opt, int classes) : o(opt), K(classes) {}
  __device__ bool valid(int64_t t) const { return ce_valid(t, K, o); }
  // x -> dL/dlogit in g; returns the pixel's loss with WITH_LOSS (one softmax for both: the fused form)
  template <bool WITH_LOSS, int KK>
  __device__ float grad_loss_(float (&x)[KK], int64_t t, float (&g)[KK]) const {
    const int y = (int)t;
    float L = 0.f;
    const float inv = 1.f / ce_softmax<KK, WITH_LOSS>(x, y, o, L);
#pragma unroll
    for (int k = 0; k < KK; ++k) g[k] = x[k] * inv - (k == y ? o.keep : 0.f) - o.uni;
    return L;
  }
  template <int KK>
  __device__ void grad(float (&x)[KK], int64_t t, float (&g)[KK]) const { grad_loss_<false>(x, t, g); }
  template <int KK>
  __device__ float grad_loss(float (&x)[KK], int64_t t, float (&g)[KK]) const { return grad_loss_<true>(x, t, g); }
  template <int KK>
  __device__ float loss(float (&x)[KK], int64_t t) const {
    float L;
    ce_softmax<KK, true>(x, (int)t, o, L);
    return L;
  }
};
typedef LowresArgs<CeOpt> CeTile;

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

// ---- low resolution (forward workspace: 1024 pixels per workgroup)
extern "C" int64_t gdl_soft_ce_lowres_workspace(int B, int K, int Ho, int Wo) {
  (void)K;
  return (int64_t)lowres_fwd_blocks((int64_t)B * Ho * Wo) * (int64_t)sizeof(double);
}

extern "C" int gdl_soft_ce_lowres_fwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo, float smooth,
                                      int has_ignore, int64_t ignore, int mean, float* loss, void* ws, int64_t ws_bytes,
                                      gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && loss && ws, "gdl_soft_ce_lowres_fwd: null pointer");
  LOWRES_SHAPE("gdl_soft_ce_lowres_fwd", K);
  GDL_CHECK_ARG(ws_bytes >= gdl_soft_ce_lowres_workspace(B, K, Ho, Wo) && (uintptr_t)ws % 8 == 0,
                "gdl_soft_ce_lowres_fwd: workspace too small or misaligned");
  CE_OPT("gdl_soft_ce_lowres_fwd", K);
  const int64_t total = (int64_t)B * Ho * Wo;
  hipStream_t s = (hipStream_t)stream;
  int nblk;
  const int rc = lowres_launch_partial<CePix>(low, target, B, K, Hi, Wi, Ho, Wo, (double*)ws, o, nblk, s);
  if (rc != GDL_OK) return rc;
  hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, nblk, mean ? 1.0 / (double)total : 1.0, loss);
  GDL_CHECK_LAUNCH("gdl_soft_ce_lowres_fwd");
  return GDL_OK;
}

static std::atomic<int> g_ce_tiled{1};
extern "C" void gdl_debug_set_soft_ce_lowres_tiled(int on) { g_ce_tiled = on; }   // A/B hook: 0 = the gather kernel for every class count

// bytes of scratch gdl_soft_ce_lowres_bwd needs (0: none -- the gather kernel)
extern "C" int64_t gdl_soft_ce_lowres_bwd_workspace(int B, int K, int Hi, int Wi, int Ho, int Wo) {
  return g_ce_tiled ? lowres_bwd_need(K, false, B, Hi, Wi, Ho, Wo) : 0;
}

extern "C" int gdl_soft_ce_lowres_bwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo, float smooth,
                                      int has_ignore, int64_t ignore, int mean, const float* upstream, float grad_scale, float* dlow,
                                      float* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && dlow, "gdl_soft_ce_lowres_bwd: null pointer");
  LOWRES_SHAPE("gdl_soft_ce_lowres_bwd", K);
  CE_OPT("gdl_soft_ce_lowres_bwd", K);
  const int64_t npix = (int64_t)B * Ho * Wo;
  const float scale = (float)(mean ? (double)grad_scale / (double)npix : (double)grad_scale);
  CeTile a = lowres_args(low, target, B, Hi, Wi, Ho, Wo, upstream, scale, nullptr, dlow, o);
  return lowres_bwd<CePix>("gdl_soft_ce_lowres_bwd", a, K, g_ce_tiled ? GDL_FOCAL_AUTO : GDL_FOCAL_GATHER, ws, ws_bytes, (hipStream_t)stream);
}

// ---- fused form: the forward leaves the unscaled patches of d(low) in `state`; the backward only reduces them.
// state = [tiles f64 loss partials | tiles * ny * nx * K f32 patches]; 0 bytes: the shape does not take this form (K > 8 or a
// resize too close to 1:1 for the tile's LDS tables) and the caller uses gdl_soft_ce_lowres_fwd / _bwd.
extern "C" int64_t gdl_soft_ce_lowres_fused_state(int B, int K, int Hi, int Wi, int Ho, int Wo) {
  int ny, nx;
  if (B <= 0 || K < 1 || Hi <= 0 || Wi <= 0 || Ho < Hi || Wo < Wi || !lowres_tile_dims(K, Hi, Wi, Ho, Wo, ny, nx)) return 0;
  if ((Ho + Hi - 1) / Hi > LOWRES_MAX_FACTOR || (Wo + Wi - 1) / Wi > LOWRES_MAX_FACTOR) return 0;
  const int64_t tiles = lowres_tiles(B, Ho, Wo);
  return tiles * (int64_t)sizeof(double) + tiles * ny * nx * K * (int64_t)sizeof(float);
}

static int ce_fused_args(const char* who, void* state, int64_t state_bytes, int B, int K, int Hi, int Wi, int Ho, int Wo, CeTile& a) {
  int ny, nx;
  const int64_t need = gdl_soft_ce_lowres_fused_state(B, K, Hi, Wi, Ho, Wo);
  GDL_CHECK_ARG(need > 0 && lowres_tile_dims(K, Hi, Wi, Ho, Wo, ny, nx), "%s: this shape does not take the fused form", who);
  GDL_CHECK_ARG(state && state_bytes >= need && (uintptr_t)state % 8 == 0, "%s: state buffer too small or misaligned", who);
  a.tile_loss = (double*)state;
  a.patches = (float*)((char*)state + lowres_tiles(B, Ho, Wo) * (int64_t)sizeof(double));
  lowres_tile_shape(a, B, Hi, Wi, Ho, Wo, ny, nx);
  return GDL_OK;
}

extern "C" int gdl_soft_ce_lowres_fused_fwd(const float* low, const int64_t* target, int B, int K, int Hi, int Wi, int Ho, int Wo,
                                            float smooth, int has_ignore, int64_t ignore, int mean, float* loss, void* state,
                                            int64_t state_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && loss, "gdl_soft_ce_lowres_fused_fwd: null pointer");
  LOWRES_SHAPE("gdl_soft_ce_lowres_fused_fwd", K);
  CE_OPT("gdl_soft_ce_lowres_fused_fwd", K);
  CeTile a{};
  int rc = ce_fused_args("gdl_soft_ce_lowres_fused_fwd", state, state_bytes, B, K, Hi, Wi, Ho, Wo, a);
  if (rc != GDL_OK) return rc;
  a.low = low; a.target = target; a.upstream = nullptr; a.dlow = nullptr; a.scale = 1.f; a.o = o;
  hipStream_t st = (hipStream_t)stream;
  rc = lowres_launch_tiles<CePix, true>(a, K, st);
  if (rc != GDL_OK) return rc;
  const int64_t npix = (int64_t)B * Ho * Wo;
  hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(256), 0, st, (const double*)a.tile_loss, (int)lowres_tiles(B, Ho, Wo),
                     mean ? 1.0 / (double)npix : 1.0, loss);
  GDL_CHECK_LAUNCH("gdl_soft_ce_lowres_fused_fwd");
  return GDL_OK;
}

extern "C" int gdl_soft_ce_lowres_fused_bwd(const void* state, int64_t state_bytes, int B, int K, int Hi, int Wi, int Ho, int Wo, int mean,
                                            const float* upstream, float grad_scale, float* dlow, gdl_stream_t stream) {
  GDL_CHECK_ARG(dlow, "gdl_soft_ce_lowres_fused_bwd: null pointer");
  LOWRES_SHAPE("gdl_soft_ce_lowres_fused_bwd", K);
  CeTile a{};
  const int rc = ce_fused_args("gdl_soft_ce_lowres_fused_bwd", const_cast<void*>(state), state_bytes, B, K, Hi, Wi, Ho, Wo, a);
  if (rc != GDL_OK) return rc;
  const int64_t npix = (int64_t)B * Ho * Wo;
  a.low = nullptr; a.target = nullptr; a.upstream = upstream; a.dlow = dlow;
  a.scale = (float)(mean ? (double)grad_scale / (double)npix : (double)grad_scale);
  a.o = CeOpt{1.f, 0.f, 0, 0};
  const int rc2 = lowres_launch_reduce(a, K, (hipStream_t)stream);
  if (rc2 != GDL_OK) return rc2;
  GDL_CHECK_LAUNCH("gdl_soft_ce_lowres_fused_bwd");
  return GDL_OK;
}
