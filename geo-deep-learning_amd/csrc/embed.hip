// The input side of the models: im2col for the few-band patch embeds, DOFA's dynamic patch-embed kernel packing and its gradient,
// the sin / cos wavelength embedding, and the normalisation of raw samples (the expressions shared with scene.hip: infer_expr.h).
#include <type_traits>

#include "gdl_common.h"
#include "infer_expr.h"

namespace {

// ------------------------------------------------------------------ DOFA patch embed helpers
// im2col for conv2d(kernel P, stride, padding pad) on NCHW f32 -> [B*Gh*Gw][Kpad]; only used where the
// input has too few channels for the implicit-GEMM kernel (C = 3..10 bands: DOFA patch embed, MiT stem)
template <typename T>
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ img, int B, int C, int H, int W,
                                                       int P, int stride, int pad, int Gh, int Gw, void* cols, int Kpad) {
  const int64_t total = (int64_t)B * Gh * Gw * Kpad;
  const int K = C * P * P;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int kk = (int)(i % Kpad);
    int64_t t = i / Kpad;
    const int gx = (int)(t % Gw); t /= Gw;
    const int gy = (int)(t % Gh);
    const int b = (int)(t / Gh);
    float v = 0.f;
    if (kk < K) {
      const int s = kk % P, r = (kk / P) % P, c = kk / (P * P);
      const int y = gy * stride + r - pad, x = gx * stride + s - pad;
      if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)
        v = img[(((int64_t)b * C + c) * H + y) * W + x];
    }
    ElemIO<T>::store(cols, i, v);
  }
}

// Same, four consecutive k per thread (Kpad % 4 == 0): ONE index decomposition per 4 outputs, (s, r, c) advanced
// incrementally, one 8- or 16-byte store.  The element-per-thread form spent its time in integer divisions (1.4 ms for the
// 671 MB of the ResNet 7x7 / stride-2 stem at batch 32).
template <typename T>
__global__ __launch_bounds__(256) void patchify4_kernel(const float* __restrict__ img, int B, int C, int H, int W,
                                                        int P, int stride, int pad, int Gh, int Gw, void* cols, int Kpad) {
  const int kq = Kpad >> 2;
  const int64_t total = (int64_t)B * Gh * Gw * kq;
  const int K = C * P * P;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int kk = (int)(i % kq) * 4;
    int64_t t = i / kq;
    const int gx = (int)(t % Gw); t /= Gw;
    const int gy = (int)(t % Gh);
    const int b = (int)(t / Gh);
    int s = kk % P, r = (kk / P) % P, c = kk / (P * P);
    const int y0 = gy * stride - pad, x0 = gx * stride - pad;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int y = y0 + r, x = x0 + s;
      v[e] = (kk + e < K && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)
                 ? img[(((int64_t)b * C + c) * H + y) * W + x] : 0.f;
      if (++s == P) { s = 0; if (++r == P) { r = 0; ++c; } }
    }
    if constexpr (std::is_same<T, float>::value)
      *(float4*)((float*)cols + i * 4) = make_float4(v[0], v[1], v[2], v[3]);
    else
      *(uint2*)((uint16_t*)cols + i * 4) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
  }
}

// generated kernel G [C][P*P][D] f32 (dofa_v2.py:157-166) -> conv weight [D][Kpad] (k = c*P*P + rs), * scaler
template <typename T>
__global__ __launch_bounds__(256) void dofa_pack_kernel(const float* __restrict__ g, int C, int PP, int D,
                                                        float scaler, void* out, int Kpad) {
  const int64_t total = (int64_t)D * Kpad;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int kk = (int)(i % Kpad), d = (int)(i / Kpad);
    float v = 0.f;
    if (kk < C * PP) v = g[(int64_t)kk * D + d] * scaler;
    ElemIO<T>::store(out, i, v);
  }
}

// backward of the pack: dG[kk][d] = scaler * dW[d][kk] for kk < C*P*P (f32)
__global__ __launch_bounds__(256) void dofa_unpack_grad_kernel(const float* __restrict__ dw, int CPP, int D, float scaler,
                                                               int Kpad, float* __restrict__ dg) {
  const int64_t total = (int64_t)CPP * D;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int d = (int)(i % D), kk = (int)(i / D);
    dg[i] = dw[(int64_t)d * Kpad + kk] * scaler;
  }
}

// ------------------------------------------------------------------ sample normalisation
__global__ __launch_bounds__(256) void normalize_u8_kernel(const uint8_t* __restrict__ in, float* out, int C,
                                                           int64_t HW, int64_t total4, const float* __restrict__ mean,
                                                           const float* __restrict__ stdv) {
  // 4 pixels per thread (HW % 4 == 0): (x/255 - mean)/std exactly as utils/tensors.py:10-35
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(((i * 4) / HW) % C);
    const uchar4 u = *(const uchar4*)(in + i * 4);
    const float m = mean[c], s = stdv[c];
    float4 o;
    o.x = ((float)u.x / 255.0f - m) / s; o.y = ((float)u.y / 255.0f - m) / s;
    o.z = ((float)u.z / 255.0f - m) / s; o.w = ((float)u.w / 255.0f - m) / s;
    *(float4*)(out + i * 4) = o;
  }
}

// same arithmetic for any raw sample dtype the reference's `.float()` accepts (uint8 / uint16 / int16 / f32)
template <typename TI>
__global__ __launch_bounds__(256) void normalize_raw_kernel(const TI* __restrict__ in, float* out, int C, int64_t HW,
                                                            int64_t total, const float* __restrict__ mean,
                                                            const float* __restrict__ stdv) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)((i / HW) % C);
    out[i] = ((float)in[i] / 255.0f - mean[c]) / stdv[c];
  }
}

// The caller's sensor range instead of 0..255 -> 0..1 (tools/script_model.py:45-52 with any image_min / image_max / norm_min /
// norm_max): normalize_range_value of infer_expr.h per element (gdl_scene_cut evaluates the same function).
// V elements of the flat NCHW tile per thread (V == 4: one
// vector load and one 16-byte store; a group may straddle a channel when H*W % 4 != 0, so the channel advances per element); the
// total % V elements behind the last whole group are done one per thread by the first threads of the grid.
template <typename TI, int V>
__global__ __launch_bounds__(256) void normalize_range_kernel(const TI* __restrict__ in, float* __restrict__ out, int C, int64_t HW,
                                                              int64_t total, float imin, float span, float d, float nmin,
                                                              const float* __restrict__ mean, const float* __restrict__ stdv) {
  struct alignas(sizeof(TI) * V) Vec { TI v[V]; };
  struct alignas(sizeof(float) * V) VecF { float v[V]; };
  const int64_t groups = total / V;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t g = tid; g < groups; g += (int64_t)gridDim.x * 256) {
    const int64_t i0 = g * V, q = i0 / HW;
    int64_t r = i0 - q * HW;
    int c = (int)(q % C);
    const Vec x = *(const Vec*)(in + i0);
    VecF o;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      o.v[e] = normalize_range_value((float)x.v[e], imin, span, d, nmin, mean[c], stdv[c]);
      if (++r == HW) { r = 0; if (++c == C) c = 0; }
    }
    *(VecF*)(out + i0) = o;
  }
  const int64_t i = groups * V + tid;
  if (i < total) {
    const int c = (int)((i / HW) % C);
    out[i] = normalize_range_value((float)in[i], imin, span, d, nmin, mean[c], stdv[c]);
  }
}

// position_embedding (dofa_v2.py:9-35): out[m, :D/2] = sin(pos*omega), out[m, D/2:] = cos(pos*omega).
// The frequency table omega[D/2] (a constant of the module) comes from the host so that the only
// difference to the reference is the sin/cos implementation (angles reach ~2000 rad).
__global__ void sincos_embed_kernel(const float* __restrict__ pos, const float* __restrict__ omega_tab,
                                    int M, int D, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = D / 2;
  if (i >= M * half) return;
  const int m = i / half, d = i - m * half;
  const float v = pos[m] * omega_tab[d];
  out[(int64_t)m * D + d] = sinf(v);
  out[(int64_t)m * D + half + d] = cosf(v);
}

}  // namespace

extern "C" int gdl_patchify(const float* img, int B, int C, int H, int W, int P, int stride, int pad, int Gh, int Gw,
                            void* cols, int out_dtype, int Kpad, gdl_stream_t stream) {
  GDL_CHECK_ARG(img && cols && Kpad >= C * P * P, "gdl_patchify: bad args");
  const int64_t total = (int64_t)B * Gh * Gw * Kpad;
  if (Kpad % 4 == 0 && (uintptr_t)cols % 16 == 0) {
    if (out_dtype == GDL_BF16)
      hipLaunchKernelGGL(patchify4_kernel<bf16_tag>, dim3(grid_for(total / 4)), dim3(256), 0, (hipStream_t)stream, img, B, C, H, W, P, stride, pad, Gh, Gw, cols, Kpad);
    else
      hipLaunchKernelGGL(patchify4_kernel<float>, dim3(grid_for(total / 4)), dim3(256), 0, (hipStream_t)stream, img, B, C, H, W, P, stride, pad, Gh, Gw, cols, Kpad);
  } else if (out_dtype == GDL_BF16)
    hipLaunchKernelGGL(patchify_kernel<bf16_tag>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, img, B, C, H, W, P, stride, pad, Gh, Gw, cols, Kpad);
  else
    hipLaunchKernelGGL(patchify_kernel<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, img, B, C, H, W, P, stride, pad, Gh, Gw, cols, Kpad);
  GDL_CHECK_LAUNCH("gdl_patchify");
  return GDL_OK;
}

extern "C" int gdl_dofa_pack_kernel(const float* g, int C, int PP, int D, float scaler, void* out, int out_dtype, int Kpad,
                                    gdl_stream_t stream) {
  GDL_CHECK_ARG(g && out && Kpad >= C * PP, "gdl_dofa_pack_kernel: bad args");
  const int64_t total = (int64_t)D * Kpad;
  if (out_dtype == GDL_BF16)
    hipLaunchKernelGGL(dofa_pack_kernel<bf16_tag>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, g, C, PP, D, scaler, out, Kpad);
  else
    hipLaunchKernelGGL(dofa_pack_kernel<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, g, C, PP, D, scaler, out, Kpad);
  GDL_CHECK_LAUNCH("gdl_dofa_pack_kernel");
  return GDL_OK;
}

extern "C" int gdl_dofa_unpack_grad(const float* dw, int C, int PP, int D, float scaler, int Kpad, float* dg,
                                    gdl_stream_t stream) {
  GDL_CHECK_ARG(dw && dg && Kpad >= C * PP, "gdl_dofa_unpack_grad: bad args");
  const int64_t total = (int64_t)C * PP * D;
  hipLaunchKernelGGL(dofa_unpack_grad_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, dw, C * PP, D, scaler, Kpad, dg);
  GDL_CHECK_LAUNCH("gdl_dofa_unpack_grad");
  return GDL_OK;
}

extern "C" int gdl_sincos_embed(const float* pos, const float* omega, int M, int D, float* out, gdl_stream_t stream) {
  GDL_CHECK_ARG(pos && omega && out && D % 2 == 0 && M > 0, "gdl_sincos_embed: bad args");
  const int total = M * (D / 2);
  hipLaunchKernelGGL(sincos_embed_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, pos, omega, M, D, out);
  GDL_CHECK_LAUNCH("gdl_sincos_embed");
  return GDL_OK;
}

extern "C" int gdl_normalize_u8(const uint8_t* in, float* out, int B, int C, int64_t HW, const float* mean,
                                const float* stdv, gdl_stream_t stream) {
  GDL_CHECK_ARG(in && out && mean && stdv, "gdl_normalize_u8: null pointer");
  GDL_CHECK_ARG(HW % 4 == 0, "gdl_normalize_u8: H*W must be a multiple of 4");
  const int64_t total4 = (int64_t)B * C * HW / 4;
  hipLaunchKernelGGL(normalize_u8_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, in, out, C, HW, total4, mean, stdv);
  GDL_CHECK_LAUNCH("gdl_normalize_u8");
  return GDL_OK;
}

extern "C" int gdl_normalize_raw(const void* in, int kind, float* out, int B, int C, int64_t HW, const float* mean,
                                 const float* stdv, gdl_stream_t stream) {
  GDL_CHECK_ARG(in && out && mean && stdv, "gdl_normalize_raw: null pointer");
  GDL_CHECK_ARG(kind >= GDL_RAW_U8 && kind <= GDL_RAW_F32, "gdl_normalize_raw: bad sample kind %d", kind);
  if (kind == GDL_RAW_U8 && HW % 4 == 0 && (uintptr_t)in % 4 == 0)
    return gdl_normalize_u8((const uint8_t*)in, out, B, C, HW, mean, stdv, stream);
  const int64_t total = (int64_t)B * C * HW;
  hipStream_t s = (hipStream_t)stream;
#define NR(T) hipLaunchKernelGGL(normalize_raw_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, (const T*)in, out, C, HW, total, mean, stdv)
  if (kind == GDL_RAW_U8) NR(uint8_t);
  else if (kind == GDL_RAW_U16) NR(uint16_t);
  else if (kind == GDL_RAW_I16) NR(int16_t);
  else NR(float);
#undef NR
  GDL_CHECK_LAUNCH("gdl_normalize_raw");
  return GDL_OK;
}

extern "C" int gdl_normalize_range(const void* in, int kind, float* out, int B, int C, int64_t HW, int image_min, int image_max,
                                   double norm_min, double norm_max, const float* mean, const float* stdv, gdl_stream_t stream) {
  GDL_CHECK_ARG(in && out && mean && stdv, "gdl_normalize_range: null pointer");
  GDL_CHECK_ARG(kind >= GDL_RAW_U8 && kind <= GDL_RAW_F32, "gdl_normalize_range: bad sample kind %d", kind);
  GDL_CHECK_ARG(B > 0 && C > 0 && HW > 0, "gdl_normalize_range: bad sizes");
  GDL_CHECK_ARG(image_max != image_min, "gdl_normalize_range: image_max == image_min (%d): the range is empty", image_min);
  const int64_t total = (int64_t)B * C * HW;
  // the scalars as Python forms them before they meet the f32 tensor: differences in int / double, one rounding to f32 each
  const RangeScalars r = range_scalars(image_min, image_max, norm_min, norm_max);
  const float imin = r.imin, span = r.span, d = r.d, nmin = r.nmin;
  const bool vec = (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0;
  hipStream_t s = (hipStream_t)stream;
#define NR(T)                                                                                                                      \
  if (vec) hipLaunchKernelGGL((normalize_range_kernel<T, 4>), dim3(grid_for(total / 4)), dim3(256), 0, s, (const T*)in, out, C, HW,  \
                              total, imin, span, d, nmin, mean, stdv);                                                             \
  else hipLaunchKernelGGL((normalize_range_kernel<T, 1>), dim3(grid_for(total)), dim3(256), 0, s, (const T*)in, out, C, HW, total, \
                          imin, span, d, nmin, mean, stdv)
  if (kind == GDL_RAW_U8) { NR(uint8_t); }
  else if (kind == GDL_RAW_U16) { NR(uint16_t); }
  else if (kind == GDL_RAW_I16) { NR(int16_t); }
  else { NR(float); }
#undef NR
  GDL_CHECK_LAUNCH("gdl_normalize_range");
  return GDL_OK;
}
