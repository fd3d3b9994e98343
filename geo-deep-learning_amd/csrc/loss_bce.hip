// Binary cross-entropy on logits with label smoothing: smp 0.5.0 SoftBCEWithLogitsLoss (losses/soft_bce.py) on
// F.binary_cross_entropy_with_logits(y_pred, t, weight, pos_weight=pos_weight, reduction="none").
//
// Per element, for logit x, raw target y (a VALUE: any fraction is legal), w / p = the weight / pos_weight of the element's channel
// (1 when absent), s = smooth_factor:
//   t     = (1 - y) s + y (1 - s)                              (y without smoothing)
//   l     = w ((1 - t) x + (1 + (p - 1) t) softplus(-x)),      softplus(-x) = max(-x, 0) + log1p(exp(-|x|))
//   dl/dx = w ((1 - t)   - (1 + (p - 1) t) sigmoid(-x)),       sigmoid(-x) from the same e = exp(-|x|), as focal_elem
//   loss  = scale * sum over the elements with y != ignore_index of l;  scale = 1 / (ALL elements, ignored ones included) for
//           "mean" (smp's loss.mean()), 1 for "sum": the host knows it, so there is no device-side divisor.
// With c = 1 + (p - 1) t both expressions are evaluated on the side of x where no two large terms cancel:
//   x >= 0:  l = w ((1 - t) x + c lp),  dl/dx = w ((1 - t) - c e r)        lp = log1p(e), r = 1 / (1 + e)
//   x <  0:  l = w (p t |x| + c lp),    dl/dx = w (c e r - p t)            ((1 - t) - c = -p t)
// which is the formula above term by term.  The ignore test is on the RAW target, before smoothing: int64 compare for an int64
// target, float compare (torch's) for an f32 one.  An ignored element is a select, not a product: it adds exactly 0 and gets an
// exactly zero gradient whatever its logit holds.
//
// Conventions as loss_focal.hip: no float atomics (same input -> same bits on every launch), per-workgroup f64 partials that one
// workgroup adds in a fixed order, the final scale applied ON THE DEVICE, nothing synchronises with the host.
//   full resolution -- NCHW f32 logits [B, C, H, W], any C >= 1 (elementwise), one element per thread-iteration, the channel of
//                      element i is (i / HW) % C (only formed where weight or pos_weight vary over channels).
//   low resolution  -- the one-class head's map [B, Hi, Wi, 1] and a target at [Ho, Wo], the bilinear logit evaluated on the fly
//                      (bilinear_index.h); the forward is a partial-sum pass, the backward recomputes in the tile or the gather
//                      form: the skeletons of lowres_tile.h with the policy BcePix.
// Every kernel is instantiated for an int64 and an f32 target (GDL_BCE_TARGET_*): neither task needs a conversion pass.
#include "gdl_common.h"
#include "bilinear_index.h"
#include "lowres_tile.h"

namespace {

struct BceOpt {
  int has_smooth;
  float smooth;
  int has_ignore;
  int64_t ignore;
  float ignore_f;           // `ignore` as the f32 targets compare it
  const float* weight;      // device, wn in {1, C}; null: 1
  const float* pos_weight;  // device, pn in {1, C}; null: 1
  int wn, pn;
  float scale;              // the reduction scale: 1 / numel ("mean") or 1 ("sum")
};

__device__ __forceinline__ bool bce_valid(int64_t y, const BceOpt& o) { return !(o.has_ignore && y == o.ignore); }
__device__ __forceinline__ bool bce_valid(float y, const BceOpt& o) { return !(o.has_ignore && y == o.ignore_f); }

// one element: its loss (LOSS) or dl/dx (otherwise), see the top of the file
template <bool LOSS>
__device__ __forceinline__ float bce_elem(float x, float y, float w, float p, const BceOpt& o) {
  const float t = o.has_smooth ? (1.f - y) * o.smooth + y * (1.f - o.smooth) : y;
  const float c = 1.f + (p - 1.f) * t;
  const float ax = fabsf(x), e = expf(-ax);
  if (LOSS) {
    const float lp = log1pf(e);
    return w * ((x >= 0.f ? (1.f - t) * ax : p * t * ax) + c * lp);
  }
  const float q = c * e / (1.f + e);
  return w * (x >= 0.f ? (1.f - t) - q : q - p * t);
}

// the weight / pos_weight of channel ch (the scalars are hoisted by the callers where neither varies)
__device__ __forceinline__ void bce_channel(const BceOpt& o, int ch, float& w, float& p) {
  w = o.weight ? o.weight[o.wn > 1 ? ch : 0] : 1.f;
  p = o.pos_weight ? o.pos_weight[o.pn > 1 ? ch : 0] : 1.f;
}

// ------------------------------------------------------------------ full resolution
// ws[0 .. gridDim.x) = loss partials
template <typename T>
__global__ __launch_bounds__(256) void bce_partial_kernel(const float* __restrict__ logits, const T* __restrict__ target, int C, int64_t HW,
                                                          int64_t total, double* __restrict__ ws, const BceOpt o) {
  const bool per_channel = o.wn > 1 || o.pn > 1;
  float w, p;
  bce_channel(o, 0, w, p);
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const T y = target[i];
    const float x = logits[i];
    if (!bce_valid(y, o)) continue;
    if (per_channel) bce_channel(o, (int)((i / HW) % C), w, p);
    acc += (double)bce_elem<true>(x, (float)y, w, p, o);
  }
  block256_store_sum(acc, ws);
}

// one workgroup: the sum of n partials in a fixed order (strided per thread, then a tree); loss = sum * scale
__global__ __launch_bounds__(256) void bce_final_kernel(const double* __restrict__ ws, int n, float scale, float* __restrict__ loss) {
  __shared__ double part[256];
  const int t = threadIdx.x;
  double acc = 0.0;
#pragma unroll 8
  for (int i = t; i < n; i += 256) acc += ws[i];
  part[t] = acc;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) part[t] += part[t + s];
    __syncthreads();
  }
  if (t == 0) loss[0] = (float)(part[0] * (double)scale);
}

template <typename T>
__global__ __launch_bounds__(256) void bce_bwd_kernel(const float* __restrict__ logits, const T* __restrict__ target, int C, int64_t HW,
                                                      int64_t total, const float* __restrict__ upstream, float grad_scale,
                                                      float* __restrict__ dlogits, int accumulate, const BceOpt o) {
  const float cf = (upstream ? upstream[0] : 1.f) * grad_scale * o.scale;
  const bool per_channel = o.wn > 1 || o.pn > 1;
  float w, p;
  bce_channel(o, 0, w, p);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const T y = target[i];
    const float x = logits[i];
    if (per_channel) bce_channel(o, (int)((i / HW) % C), w, p);
    const float v = bce_valid(y, o) ? cf * bce_elem<false>(x, (float)y, w, p, o) : 0.f;      // an ignored element: exactly zero
    dlogits[i] = accumulate ? dlogits[i] + v : v;
  }
}

// ------------------------------------------------------------------ low resolution, one class: low [B, Hi, Wi, 1]
// the policy of lowres_tile.h; T = the target's element type
template <typename T>
struct BcePix {
  typedef BceOpt Opt;
  typedef T Target;
  static constexpr bool ONE_CLASS = true, COUNTS = false;
  BceOpt o;
  float w, p;      // the one channel's weight / pos_weight
  __device__ BcePix(const BceOpt& opt, int) : o(opt) { bce_channel(o, 0, w, p); }
  __device__ bool valid(T y) const { return bce_valid(y, o); }
  __device__ void grad(const float (&x)[1], T y, float (&g)[1]) const { g[0] = bce_elem<false>(x[0], (float)y, w, p, o); }
  __device__ float loss(const float (&x)[1], T y) const { return bce_elem<true>(x[0], (float)y, w, p, o); }
};

}  // namespace

// ============================================================================ C ABI
#define BCE_OPT_PARAMS                                                                                                           \
  int has_smooth, float smooth, int has_ignore, int64_t ignore, float ignore_f, const float* weight, int weight_numel,          \
      const float* pos_weight, int pos_weight_numel, float scale

static int bce_host_opt(const char* who, int C, BCE_OPT_PARAMS, BceOpt& o) {
  GDL_CHECK_ARG(C >= 1, "%s: C=%d channels", who, C);
  GDL_CHECK_ARG(!has_smooth || (smooth >= 0.f && smooth <= 1.f), "%s: smooth_factor %g outside [0, 1]", who, (double)smooth);
  GDL_CHECK_ARG(scale > 0.f && scale <= 3.0e38f, "%s: the reduction scale %g must be finite and > 0", who, (double)scale);
  GDL_CHECK_ARG(!weight || weight_numel == 1 || weight_numel == C, "%s: weight of %d values for C=%d channels (1 or C)", who,
                weight_numel, C);
  GDL_CHECK_ARG(!pos_weight || pos_weight_numel == 1 || pos_weight_numel == C, "%s: pos_weight of %d values for C=%d channels (1 or C)",
                who, pos_weight_numel, C);
  o.has_smooth = has_smooth != 0;
  o.smooth = has_smooth ? smooth : 0.f;
  o.has_ignore = has_ignore != 0;
  o.ignore = ignore;
  o.ignore_f = ignore_f;
  o.weight = weight;
  o.pos_weight = pos_weight;
  o.wn = weight ? weight_numel : 1;
  o.pn = pos_weight ? pos_weight_numel : 1;
  o.scale = scale;
  return GDL_OK;
}
#define BCE_OPT(who, C)                                                                                                          \
  BceOpt o;                                                                                                                      \
  { const int st_ = bce_host_opt(who, C, has_smooth, smooth, has_ignore, ignore, ignore_f, weight, weight_numel, pos_weight,     \
                                 pos_weight_numel, scale, o);                                                                    \
    if (st_ != GDL_OK) return st_; }
#define BCE_TARGET_TYPE(who) \
  GDL_CHECK_ARG(target_type == GDL_BCE_TARGET_I64 || target_type == GDL_BCE_TARGET_F32, who ": unknown target type %d", target_type)
// `__VA_ARGS__` with TT = the target's element type
#define BCE_TYPE_SWITCH(...)                                               \
  if (target_type == GDL_BCE_TARGET_I64) { typedef int64_t TT; __VA_ARGS__; } \
  else { typedef float TT; __VA_ARGS__; }

// (2048 elements per workgroup up to 2048 workgroups, as gdl_focal_fwd: a streaming read wants every SIMD full)
static int bce_blocks(int64_t total, int per_block) {
  int64_t g = (total + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

#define BCE_FULL_SHAPE(who) \
  GDL_CHECK_ARG(B > 0 && C > 0 && HW > 0 && (int64_t)B * C <= ((int64_t)1 << 62) / HW, who ": bad sizes")

extern "C" int64_t gdl_soft_bce_workspace(int B, int C, int64_t HW) {
  if (B <= 0 || C <= 0 || HW <= 0) return 0;
  return (int64_t)bce_blocks((int64_t)B * C * HW, 2048) * (int64_t)sizeof(double);
}

extern "C" int gdl_soft_bce_fwd(const float* logits, const void* target, int target_type, int B, int C, int64_t HW, BCE_OPT_PARAMS,
                                float* loss, void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && loss && ws, "gdl_soft_bce_fwd: null pointer");
  BCE_FULL_SHAPE("gdl_soft_bce_fwd");
  BCE_TARGET_TYPE("gdl_soft_bce_fwd");
  GDL_CHECK_ARG(ws_bytes >= gdl_soft_bce_workspace(B, C, HW) && (uintptr_t)ws % 8 == 0,
                "gdl_soft_bce_fwd: workspace too small or misaligned");
  BCE_OPT("gdl_soft_bce_fwd", C);
  const int64_t total = (int64_t)B * C * HW;
  const int nblk = bce_blocks(total, 2048);
  hipStream_t s = (hipStream_t)stream;
  BCE_TYPE_SWITCH(hipLaunchKernelGGL((bce_partial_kernel<TT>), dim3(nblk), dim3(256), 0, s, logits, (const TT*)target, C, HW, total,
                                     (double*)ws, o));
  hipLaunchKernelGGL(bce_final_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, nblk, o.scale, loss);
  GDL_CHECK_LAUNCH("gdl_soft_bce_fwd");
  return GDL_OK;
}

extern "C" int gdl_soft_bce_bwd(const float* logits, const void* target, int target_type, int B, int C, int64_t HW, BCE_OPT_PARAMS,
                                const float* upstream, float grad_scale, float* dlogits, int accumulate, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && dlogits, "gdl_soft_bce_bwd: null pointer");
  BCE_FULL_SHAPE("gdl_soft_bce_bwd");
  BCE_TARGET_TYPE("gdl_soft_bce_bwd");
  BCE_OPT("gdl_soft_bce_bwd", C);
  const int64_t total = (int64_t)B * C * HW;
  BCE_TYPE_SWITCH(hipLaunchKernelGGL((bce_bwd_kernel<TT>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, logits,
                                     (const TT*)target, C, HW, total, upstream, grad_scale, dlogits, accumulate, o));
  GDL_CHECK_LAUNCH("gdl_soft_bce_bwd");
  return GDL_OK;
}

// ---- low resolution, one class: the shape limits of gdl_focal_binary_lowres_* (forward workspace: 1024 pixels per workgroup)
extern "C" int64_t gdl_soft_bce_lowres_workspace(int B, int Ho, int Wo) {
  if (B <= 0 || Ho <= 0 || Wo <= 0) return 0;
  return (int64_t)lowres_fwd_blocks((int64_t)B * Ho * Wo) * (int64_t)sizeof(double);
}

extern "C" int gdl_soft_bce_lowres_fwd(const float* low, const void* target, int target_type, int B, int Hi, int Wi, int Ho, int Wo,
                                       BCE_OPT_PARAMS, float* loss, void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && loss && ws, "gdl_soft_bce_lowres_fwd: null pointer");
  LOWRES_SHAPE("gdl_soft_bce_lowres_fwd", 1);
  BCE_TARGET_TYPE("gdl_soft_bce_lowres_fwd");
  GDL_CHECK_ARG(ws_bytes >= gdl_soft_bce_lowres_workspace(B, Ho, Wo) && (uintptr_t)ws % 8 == 0,
                "gdl_soft_bce_lowres_fwd: workspace too small or misaligned");
  BCE_OPT("gdl_soft_bce_lowres_fwd", 1);
  hipStream_t s = (hipStream_t)stream;
  int nblk;
  BCE_TYPE_SWITCH(lowres_launch_partial<BcePix<TT>>(low, target, B, 1, Hi, Wi, Ho, Wo, (double*)ws, o, nblk, s));
  hipLaunchKernelGGL(bce_final_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, nblk, o.scale, loss);
  GDL_CHECK_LAUNCH("gdl_soft_bce_lowres_fwd");
  return GDL_OK;
}

// the final factor is upstream * (grad_scale * scale): LowresTile::scale holds the product of the two
extern "C" int gdl_soft_bce_lowres_bwd(const float* low, const void* target, int target_type, int B, int Hi, int Wi, int Ho, int Wo,
                                       BCE_OPT_PARAMS, const float* upstream, float grad_scale, float* dlow, float* ws,
                                       int64_t ws_bytes, int form, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && target && dlow, "gdl_soft_bce_lowres_bwd: null pointer");
  LOWRES_SHAPE("gdl_soft_bce_lowres_bwd", 1);
  BCE_TARGET_TYPE("gdl_soft_bce_lowres_bwd");
  GDL_CHECK_ARG(!ws || (uintptr_t)ws % 4 == 0, "gdl_soft_bce_lowres_bwd: workspace misaligned");
  BCE_OPT("gdl_soft_bce_lowres_bwd", 1);
  auto a = lowres_args(low, target, B, Hi, Wi, Ho, Wo, upstream, grad_scale * o.scale, nullptr, dlow, o);
  BCE_TYPE_SWITCH(return lowres_bwd<BcePix<TT>>("gdl_soft_bce_lowres_bwd", a, 1, form, ws, ws_bytes, (hipStream_t)stream));
}
