// The prediction tail behind the classifier head: the bilinear logit resize (forward and backward), softmax / sigmoid decisions and
// class probabilities -- from full-resolution logits or straight from the head's low-resolution map -- and the IoU counts of a mask.
// One kernel per op: KT > 0 is the class count as a compile-time constant (1..16), KT == 0 takes it from the run-time argument.
#include "gdl_common.h"
#include "bilinear_index.h"
#include "infer_expr.h"

namespace {

// Where flat index i over [B, Ho, W] lies (W = Wo, xi = ox; or W = Wo / V groups of V pixels, xi = the group) and the two source
// rows its bilinear form reads: the preamble of every kernel that resizes the low-resolution map on the fly
struct RowPos { int b, oy, xi, y0, y1; float ly; };
__device__ __forceinline__ RowPos row_pos(int64_t i, int W, int Ho, int Hi, float ry) {
  RowPos r;
  r.xi = (int)(i % W);
  const int64_t t = i / W;
  r.oy = (int)(t % Ho); r.b = (int)(t / Ho);
  src_index2(ry, r.oy, Hi, r.y0, r.y1, r.ly);
  return r;
}

// the K bilinear logits of output pixel (r.b, r.oy, ox) from the NHWC map [B, Hi, Wi, K]
template <int K>
__device__ __forceinline__ void pixel_logits(const float* __restrict__ low, const RowPos& r, int ox, int Hi, int Wi, float rx, float (&x)[K]) {
  int x0, x1; float lx;
  src_index2(rx, ox, Wi, x0, x1, lx);
  bilinear_logits<K>(low, r.b, Hi, Wi, r.y0, r.y1, x0, x1, r.ly, lx, x);
}

// softmax(dim=1).argmax(dim=1) of one pixel: first index of the maximal f32 softmax value (torch semantics); x becomes the probabilities
template <int K>
__device__ __forceinline__ int softmax_argmax_of(float (&x)[K]) {
  logits_to_probs<K>(x);
  int best = 0; float bv = x[0];
#pragma unroll
  for (int k = 1; k < K; ++k) if (x[k] > bv) { bv = x[k]; best = k; }
  return best;
}

// NHWC [B,Hi,Wi,K] f32 -> NCHW [B,K,Ho,Wo] f32, bilinear align_corners=False.  Each logit is stored as it is formed (held in an
// array first, 13 and 14 classes lose a wave per SIMD).  More than 16 classes (KT == 0): the class dimension in a run-time loop (a
// loss whose low-resolution kernels stop at 16 classes materialises its logits through this one)
template <int KT>
__global__ __launch_bounds__(256) void upsample_logits_kernel(const float* __restrict__ in, int B, int Hi, int Wi, int k_rt,
                                                              float* __restrict__ out, int Ho, int Wo) {
  const int K = KT ? KT : k_rt;
  const int64_t total = (int64_t)B * Ho * Wo;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const RowPos r = row_pos(i, Wo, Ho, Hi, ry);
    int x0, x1; float lx;
    src_index2(rx, r.xi, Wi, x0, x1, lx);
    bilinear_logits_each<KT>(in, r.b, Hi, Wi, K, r.y0, r.y1, x0, x1, r.ly, lx,
                             [&](int k, float v) { out[(((int64_t)r.b * K + k) * Ho + r.oy) * Wo + r.xi] = v; });
  }
}

// Backward of the logit upsample, separable (bilinear weights factor as wy*wx), gather form:
//   pass 1: tmp[b,k,iy,ox] = sum_oy wy(oy->iy) * dout[b,k,oy,ox]      (coalesced along ox)
//   pass 2: din[b,iy,ix,k] = sum_ox wx(ox->ix) * tmp[b,k,iy,ox]
__global__ __launch_bounds__(256) void upsample_logits_bwd_pass1(const float* __restrict__ dout, int BK, int Ho, int Wo,
                                                                 float* __restrict__ tmp, int Hi) {
  const int64_t total = (int64_t)BK * Hi * Wo;
  const float ry = (float)Hi / (float)Ho;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % Wo);
    const int64_t t = i / Wo;
    const int iy = (int)(t % Hi);
    const int64_t bk = t / Hi;
    int lo, hi;
    cand_range(iy, ry, Ho, lo, hi);
    float acc = 0.f;
    for (int oy = lo; oy <= hi; ++oy) {
      int y0, y1; float ly;
      src_index2(ry, oy, Hi, y0, y1, ly);
      const float wy = (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
      if (wy != 0.f) acc += wy * dout[(bk * Ho + oy) * Wo + ox];
    }
    tmp[i] = acc;
  }
}

template <int KT>
__global__ __launch_bounds__(256) void upsample_logits_bwd_pass2(const float* __restrict__ tmp, int B, int k_rt, int Wo,
                                                                 float* __restrict__ din, int Hi, int Wi) {
  const int K = KT ? KT : k_rt;
  const int64_t total = (int64_t)B * Hi * Wi * K;
  const float rx = (float)Wi / (float)Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int k = (int)(i % K);
    int64_t t = i / K;
    const int ix = (int)(t % Wi); t /= Wi;
    const int iy = (int)(t % Hi);
    const int b = (int)(t / Hi);
    int lo, hi;
    cand_range(ix, rx, Wo, lo, hi);
    const float* row = tmp + (((int64_t)b * K + k) * Hi + iy) * Wo;
    float acc = 0.f;
    for (int ox = lo; ox <= hi; ++ox) {
      int x0, x1; float lx;
      src_index2(rx, ox, Wi, x0, x1, lx);
      const float wx = (x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f);
      if (wx != 0.f) acc += wx * row[ox];
    }
    din[i] = acc;
  }
}

// softmax(dim=1).argmax(dim=1) of full-resolution NCHW logits
template <int K>
__global__ __launch_bounds__(256) void softmax_argmax_kernel(const float* __restrict__ logits, int B, int64_t HW,
                                                             int64_t* __restrict__ mask) {
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW, p = i - b * HW;
    float x[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = logits[(b * K + k) * HW + p];
    mask[i] = softmax_argmax_of<K>(x);
  }
}

// class probabilities of the exported inference model: softmax over the class dim (K > 1) or sigmoid (K == 1).  More than 16
// classes (KT == 0): the same softmax with the class dimension in run-time loops (the logits are read three times, never held in
// a run-time indexed array; the inference wrapper's route for a head wider than the unrolled kernels)
template <int KT>
__global__ __launch_bounds__(256) void class_probs_kernel(const float* __restrict__ logits, int B, int k_rt, int64_t HW,
                                                          float* __restrict__ probs) {
  const int K = KT ? KT : k_rt;
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / HW, p = i - b * HW;
    if constexpr (KT > 0) {
      float x[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) x[k] = logits[(b * K + k) * HW + p];
      logits_to_probs<KT>(x);
#pragma unroll
      for (int k = 0; k < KT; ++k) probs[(b * K + k) * HW + p] = x[k];
    } else {
      const float* x = logits + b * K * HW + p;
      float mx = -INFINITY, s = 0.f;
      for (int k = 0; k < K; ++k) mx = fmaxf(mx, x[k * HW]);
      for (int k = 0; k < K; ++k) s += expf(x[k * HW] - mx);
      for (int k = 0; k < K; ++k) probs[(b * K + k) * HW + p] = expf(x[k * HW] - mx) / s;
    }
  }
}

// ------------------------------------------------------------------ mask prediction from the LOW-resolution logits
// softmax(dim=1).argmax(dim=1) of the resized logits straight from the head's low-resolution map (validation / test / inference:
// `outputs.out.softmax(dim=1).argmax(dim=1)`, segmentation_dofa.py:278-281): the bilinear logits of a pixel with the expression of
// upsample_logits_kernel, then softmax_argmax_kernel's decision -- the same mask, bit for bit, without the [B, K, H, W] f32 tensor
// (335 MB written and read again at batch 64).
template <int K>
__global__ __launch_bounds__(256) void upsample_argmax_kernel(const float* __restrict__ low, int B, int Hi, int Wi, int Ho, int Wo,
                                                              int64_t* __restrict__ mask) {
  const int64_t total = (int64_t)B * Ho * Wo;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const RowPos r = row_pos(i, Wo, Ho, Hi, ry);
    float x[K];
    pixel_logits<K>(low, r, r.xi, Hi, Wi, rx, x);
    mask[i] = softmax_argmax_of<K>(x);
  }
}

// One-class prediction, `(out.sigmoid().squeeze(1) > threshold).long()` (segmentation_dofa.py:279), as one pass: the sigmoid as
// class_probs_kernel<1> writes it, 1 / (1 + exp(-x)) in f32, compared with the threshold in probability space (sigmoid(x) > 0.5 and
// x > 0 differ for 0 < x < ~1e-7, where the f32 sigmoid rounds to 0.5).
__device__ __forceinline__ int64_t sigmoid_over(float x, float th) { return 1.0f / (1.0f + expf(-x)) > th ? 1 : 0; }

__global__ __launch_bounds__(256) void sigmoid_threshold_kernel(const float* __restrict__ logits, int64_t total, float th,
                                                                int64_t* __restrict__ mask) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) mask[i] = sigmoid_over(logits[i], th);
}

// ... and straight from the one-class head's low-resolution map [B, Hi, Wi, 1]: the bilinear logit of upsample_logits_kernel per
// pixel, then the same decision -- the mask of gdl_upsample_logits + gdl_sigmoid_threshold without the [B, 1, H, W] f32 tensor.
__global__ __launch_bounds__(256) void upsample_threshold_kernel(const float* __restrict__ low, int B, int Hi, int Wi, int Ho, int Wo,
                                                                 float th, int64_t* __restrict__ mask) {
  const int64_t total = (int64_t)B * Ho * Wo;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const RowPos r = row_pos(i, Wo, Ho, Hi, ry);
    float x[1];
    pixel_logits<1>(low, r, r.xi, Hi, Wi, rx, x);
    mask[i] = sigmoid_over(x[0], th);
  }
}

// Class probabilities of the exported inference model straight from a head's low-resolution map (tools/script_model.py:53-58 over
// dofa.py:89-95): the bilinear logits of a pixel with the expression of upsample_logits_kernel, then class_probs_kernel's softmax
// (K > 1) or sigmoid (K == 1) -- the probabilities of gdl_upsample_logits + gdl_class_probs with one store per value instead of a
// store, a load and a store of [B, K, Ho, Wo] f32.  The kernel is store-bound (K * 4 bytes per pixel against a few cached reads of
// the map): a thread owns V consecutive pixels of an output row, so every class plane is written along Wo, 256 contiguous bytes
// per wave-instruction with V == 1 and 1 KiB (16 bytes per lane, the widest store there is) with V == 4, which needs Wo % 4 == 0.
template <int K, int V>
__global__ __launch_bounds__(256) void upsample_probs_kernel(const float* __restrict__ low, int B, int Hi, int Wi, int Ho, int Wo,
                                                             float* __restrict__ probs) {
  struct alignas(sizeof(float) * V) VecF { float v[V]; };
  const int Wv = Wo / V;
  const int64_t total = (int64_t)B * Ho * Wv;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const RowPos r = row_pos(i, Wv, Ho, Hi, ry);
    const int ox0 = r.xi * V;
    float x[V][K];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      pixel_logits<K>(low, r, ox0 + e, Hi, Wi, rx, x[e]);
      logits_to_probs<K>(x[e]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      VecF o;
#pragma unroll
      for (int e = 0; e < V; ++e) o.v[e] = x[e][k];
      *(VecF*)(probs + (((int64_t)r.b * K + k) * Ho + r.oy) * Wo + ox0) = o;
    }
  }
}

// ------------------------------------------------------------------ IoU counts (torchmetrics MeanIoU update)
// per sample b and class k: intersection |pred==k & target==k|, |pred==k|, |target==k| as exact 64-bit counts.
// LDS histogram per block, integer atomics only (deterministic).
__global__ __launch_bounds__(256) void iou_counts_kernel(const int64_t* __restrict__ pred,
                                                         const int64_t* __restrict__ target, int64_t P, int K,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ unsigned h[3 * 64];
  for (int i = threadIdx.x; i < 3 * K; i += 256) h[i] = 0;
  __syncthreads();
  const int b = blockIdx.y;
  const int64_t per = (P + gridDim.x - 1) / gridDim.x;
  const int64_t p0 = per * blockIdx.x, p1 = p0 + per < P ? p0 + per : P;
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
    const int64_t a = pred[(int64_t)b * P + p], t = target[(int64_t)b * P + p];
    const bool av = a >= 0 && a < K, tv = t >= 0 && t < K;
    if (av) atomicAdd(&h[K + (int)a], 1u);
    if (tv) atomicAdd(&h[2 * K + (int)t], 1u);
    if (av && a == t) atomicAdd(&h[(int)a], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * K; i += 256)
    if (h[i]) atomicAdd(&counts[((int64_t)b * 3 + i / K) * K + i % K], (unsigned long long)h[i]);
}

}  // namespace

// K_SWITCH for the kernels with a run-time-K form: more than 16 classes take instantiation 0
#define K_SWITCH_ANY(K, ...)                                   \
  if ((K) > 16) { constexpr int KK = 0; __VA_ARGS__; }         \
  else { K_SWITCH(K, __VA_ARGS__); }

extern "C" int gdl_upsample_logits(const float* in, int B, int Hi, int Wi, int K, float* out, int Ho, int Wo,
                                   gdl_stream_t stream) {
  GDL_CHECK_ARG(in && out, "gdl_upsample_logits: null pointer");
  const int64_t total = (int64_t)B * Ho * Wo;
  K_SWITCH_ANY(K, hipLaunchKernelGGL((upsample_logits_kernel<KK>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, B, Hi, Wi, K, out, Ho, Wo));
  GDL_CHECK_LAUNCH("gdl_upsample_logits");
  return GDL_OK;
}

extern "C" int64_t gdl_upsample_logits_bwd_workspace(int B, int K, int Hi, int Wo) {
  return (int64_t)B * K * Hi * Wo * (int64_t)sizeof(float);
}

extern "C" int gdl_upsample_logits_bwd(const float* dout, int B, int Ho, int Wo, int K, float* din, int Hi, int Wi,
                                       float* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(dout && din && ws, "gdl_upsample_logits_bwd: null pointer");
  GDL_CHECK_ARG(ws_bytes >= gdl_upsample_logits_bwd_workspace(B, K, Hi, Wo), "gdl_upsample_logits_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(upsample_logits_bwd_pass1, dim3(grid_for((int64_t)B * K * Hi * Wo)), dim3(256), 0, s, dout, B * K, Ho, Wo, ws, Hi);
  K_SWITCH_ANY(K, hipLaunchKernelGGL((upsample_logits_bwd_pass2<KK>), dim3(grid_for((int64_t)B * Hi * Wi * K)), dim3(256), 0, s, ws, B, K, Wo, din, Hi, Wi));
  GDL_CHECK_LAUNCH("gdl_upsample_logits_bwd");
  return GDL_OK;
}

extern "C" int gdl_softmax_argmax(const float* logits, int B, int K, int64_t HW, int64_t* mask, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && mask, "gdl_softmax_argmax: null pointer");
  const int64_t total = (int64_t)B * HW;
  K_SWITCH(K, hipLaunchKernelGGL((softmax_argmax_kernel<KK>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, logits, B, HW, mask));
  GDL_CHECK_LAUNCH("gdl_softmax_argmax");
  return GDL_OK;
}

extern "C" int gdl_upsample_argmax(const float* low, int B, int Hi, int Wi, int K, int64_t* mask, int Ho, int Wo, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && mask && B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && K >= 2, "gdl_upsample_argmax: bad args");
  const int64_t total = (int64_t)B * Ho * Wo;
  K_SWITCH(K, hipLaunchKernelGGL((upsample_argmax_kernel<KK>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, low, B, Hi, Wi, Ho, Wo, mask));
  GDL_CHECK_LAUNCH("gdl_upsample_argmax");
  return GDL_OK;
}

extern "C" int gdl_sigmoid_threshold(const float* logits, int64_t total, float threshold, int64_t* mask, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && mask && total > 0, "gdl_sigmoid_threshold: bad args");
  hipLaunchKernelGGL(sigmoid_threshold_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, logits, total, threshold, mask);
  GDL_CHECK_LAUNCH("gdl_sigmoid_threshold");
  return GDL_OK;
}

extern "C" int gdl_upsample_threshold(const float* low, int B, int Hi, int Wi, int64_t* mask, int Ho, int Wo, float threshold,
                                      gdl_stream_t stream) {
  GDL_CHECK_ARG(low && mask, "gdl_upsample_threshold: null pointer");
  GDL_CHECK_ARG(B > 0 && Hi > 0 && Wi > 0 && Ho >= Hi && Wo >= Wi, "gdl_upsample_threshold: bad sizes (an upsample is expected)");
  GDL_CHECK_ARG((Ho + Hi - 1) / Hi <= 64 && (Wo + Wi - 1) / Wi <= 64, "gdl_upsample_threshold: upsampling factors above 64 are not supported");
  const int64_t total = (int64_t)B * Ho * Wo;
  hipLaunchKernelGGL(upsample_threshold_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, low, B, Hi, Wi, Ho, Wo, threshold, mask);
  GDL_CHECK_LAUNCH("gdl_upsample_threshold");
  return GDL_OK;
}

extern "C" int gdl_class_probs(const float* logits, int B, int K, int64_t HW, float* probs, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && probs, "gdl_class_probs: null pointer");
  const int64_t total = (int64_t)B * HW;
  K_SWITCH_ANY(K, hipLaunchKernelGGL((class_probs_kernel<KK>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, logits, B, K, HW, probs));
  GDL_CHECK_LAUNCH("gdl_class_probs");
  return GDL_OK;
}

// every size pair gdl_upsample_logits takes (an upsample, a downsample or the identity, any factor); K up to the 16 unrolled classes
extern "C" int gdl_upsample_probs(const float* low, int B, int Hi, int Wi, int K, float* probs, int Ho, int Wo, gdl_stream_t stream) {
  GDL_CHECK_ARG(low && probs, "gdl_upsample_probs: null pointer");
  GDL_CHECK_ARG(B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "gdl_upsample_probs: bad sizes %d x %d x %d -> %d x %d", B, Hi, Wi, Ho, Wo);
  GDL_CHECK_ARG(K >= 1 && K <= 16, "gdl_upsample_probs: 1..16 classes, got %d (more: gdl_upsample_logits + gdl_class_probs)", K);
  hipStream_t s = (hipStream_t)stream;
  if (Wo % 4 == 0 && (uintptr_t)probs % 16 == 0) {
    K_SWITCH(K, hipLaunchKernelGGL((upsample_probs_kernel<KK, 4>), dim3(grid_for((int64_t)B * Ho * (Wo / 4))), dim3(256), 0, s, low, B, Hi, Wi, Ho, Wo, probs));
  } else {
    K_SWITCH(K, hipLaunchKernelGGL((upsample_probs_kernel<KK, 1>), dim3(grid_for((int64_t)B * Ho * Wo)), dim3(256), 0, s, low, B, Hi, Wi, Ho, Wo, probs));
  }
  GDL_CHECK_LAUNCH("gdl_upsample_probs");
  return GDL_OK;
}

extern "C" int gdl_iou_counts(const int64_t* pred, const int64_t* target, int B, int64_t P, int K, int64_t* counts,
                              gdl_stream_t stream) {
  GDL_CHECK_ARG(pred && target && counts && B > 0 && P > 0, "gdl_iou_counts: bad args");
  GDL_CHECK_ARG(K > 0 && K <= 64, "gdl_iou_counts: 1..64 classes");
  GDL_CHECK_ARG(P / 64 < (1ll << 32), "gdl_iou_counts: sample too large");
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(counts, 0, (size_t)B * 3 * K * sizeof(int64_t), s);
  int64_t chunks = (P + 65535) / 65536;
  if (chunks > 1024) chunks = 1024;
  hipLaunchKernelGGL(iou_counts_kernel, dim3((unsigned)chunks, B), dim3(256), 0, s, pred, target, P, K,
                     (unsigned long long*)counts);
  GDL_CHECK_LAUNCH("gdl_iou_counts");
  return GDL_OK;
}
