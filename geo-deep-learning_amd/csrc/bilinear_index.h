// Index arithmetic of the bilinear (align_corners=False) logit resize, shared by the kernels that evaluate it on the fly
// (predict.hip: gdl_upsample_logits, gdl_upsample_argmax, gdl_upsample_threshold, gdl_upsample_probs; loss_dice.hip: gdl_dice_loss_lowres_* and the binary forward; lowres_tile.h:
// the kernel skeletons behind gdl_soft_ce_lowres_*, gdl_focal_lowres_*, gdl_focal_binary_lowres_*, gdl_soft_bce_lowres_* and the
// binary Dice family's backward; resample_vec.h: the resize kernels of resample.hip and resize_conv_*.hip).  One definition, so that every kernel evaluates the expression gdl_upsample_logits writes.
#pragma once
#include "gdl_common.h"

namespace {

// torch area_pixel_compute_source_index(align_corners=False) + index/lambda (UpSample.h)
__device__ __forceinline__ void src_index2(float ratio, int dst, int in_size, int& i0, int& i1, float& l1) {
  float s = ratio * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
}

// output positions [lo, hi] that can interpolate from input position i (a superset; callers test the weight)
__device__ __forceinline__ void cand_range(int i, float ratio, int out_size, int& lo, int& hi) {
  lo = (int)floorf(((float)i - 0.5f) / ratio - 0.5f) - 1;
  hi = (int)ceilf(((float)i + 1.5f) / ratio - 0.5f) + 1;
  lo = lo < 0 ? 0 : lo;
  hi = hi > out_size - 1 ? out_size - 1 : hi;
}

// low-resolution index range [lo, hi] that the full-resolution positions [p0, p1] interpolate from
__device__ __forceinline__ void touched_range(float ratio, int p0, int p1, int in_size, int& lo, int& hi) {
  int a0, a1, b0, b1; float l;
  src_index2(ratio, p0, in_size, a0, a1, l);
  src_index2(ratio, p1, in_size, b0, b1, l);
  lo = a0; hi = b1;
}

// f(k, logit k) for the K bilinear logits of one output pixel from the NHWC map [B, Hi, Wi, K]: THE expression of the logit resize.
// KT > 0: K == KT classes, unrolled; KT == 0: K at run time
template <int KT, typename F>
__device__ __forceinline__ void bilinear_logits_each(const float* __restrict__ in, int b, int Hi, int Wi, int k_rt, int y0, int y1, int x0,
                                                     int x1, float ly, float lx, F f) {
  const int K = KT ? KT : k_rt;
  const float* p00 = in + (((int64_t)b * Hi + y0) * Wi + x0) * K;
  const float* p01 = in + (((int64_t)b * Hi + y0) * Wi + x1) * K;
  const float* p10 = in + (((int64_t)b * Hi + y1) * Wi + x0) * K;
  const float* p11 = in + (((int64_t)b * Hi + y1) * Wi + x1) * K;
  const float hy = 1.f - ly, hx = 1.f - lx;
  auto one = [&](int k) { f(k, hy * (hx * p00[k] + lx * p01[k]) + ly * (hx * p10[k] + lx * p11[k])); };
  if constexpr (KT > 0) {
#pragma unroll
    for (int k = 0; k < KT; ++k) one(k);
  } else {
    for (int k = 0; k < K; ++k) one(k);      // (no pragma: a full unroll of a run-time loop cannot be done and warns)
  }
}

// ... into registers, for the kernels that go on from the logits (K is a compile-time constant there)
template <int K>
__device__ __forceinline__ void bilinear_logits(const float* __restrict__ in, int b, int Hi, int Wi, int y0, int y1, int x0, int x1,
                                                float ly, float lx, float (&x)[K]) {
  bilinear_logits_each<K>(in, b, Hi, Wi, K, y0, y1, x0, x1, ly, lx, [&](int k, float v) { x[k] = v; });
}

}  // namespace
