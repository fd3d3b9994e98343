// The per-element expressions of the inference path, each defined once for the kernels that must agree on them bit for bit:
// embed.hip (gdl_normalize_range), predict.hip (gdl_class_probs, gdl_upsample_probs, the argmax kernels), scene.hip (gdl_scene_cut, gdl_scene_blend_lowres, gdl_scene_finish) and
// scene_regions.hip (gdl_scene_regions_stats).
#pragma once
#include "gdl_common.h"

namespace {

// ((d * (x - image_min)) / span + norm_min - mean[c]) / std[c] with d = norm_max - norm_min and span = image_max - image_min, every
// step rounded to f32 in the order utils/tensors.py:19-21,34 takes them on an f32 tensor (not folded into one scale and offset:
// that form differs from the reference by up to a few ulp)
__device__ __forceinline__ float normalize_range_value(float x, float imin, float span, float d, float nmin, float mean, float stdv) {
  return ((d * (x - imin)) / span + nmin - mean) / stdv;
}

// the scalars of normalize_range_value as Python forms them before they meet the f32 tensor: differences in int / double, one
// rounding to f32 each
struct RangeScalars { float imin, span, d, nmin; };
inline RangeScalars range_scalars(int image_min, int image_max, double norm_min, double norm_max) {
  return {(float)image_min, (float)((int64_t)image_max - (int64_t)image_min), (float)(norm_max - norm_min), (float)norm_min};
}

// the probability a canvas holds for one class at one pixel: the class's weighted sum over the weight sum, 0 where the pixel is
// not live (weight 0, or invalid by the plane of gdl_scene_finish_valid).  What gdl_scene_finish writes to `probs`, and what
// gdl_scene_regions_stats (scene_regions.hip) turns into a pixel's confidence.
__device__ __forceinline__ float canvas_prob(float c, float den, bool live) { return live ? c / den : 0.f; }

// K logits -> class probabilities in place: 1 / (1 + exp(-x)) for one class, otherwise the softmax with the maximum subtracted
template <int K>
__device__ __forceinline__ void logits_to_probs(float (&x)[K]) {
  if constexpr (K == 1) {
    x[0] = 1.0f / (1.0f + expf(-x[0]));
  } else {
    float mx = -INFINITY, s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, x[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) { x[k] = expf(x[k] - mx); s += x[k]; }
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = x[k] / s;
  }
}

}  // namespace
