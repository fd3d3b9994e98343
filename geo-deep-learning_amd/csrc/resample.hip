// Bilinear resize (align_corners=False) and adaptive average pooling on NHWC tensors.
// HBM-bound: one thread per (pixel, 4-channel vector); f32 arithmetic; gather formulation in
// both directions (no atomics -> deterministic backward).
// (The resized 3x3 convolutions built on the same resize are units of their own: resize_conv_fwd.hip, resize_conv_bwd.hip.)
#include "gdl_common.h"
#include "resample_vec.h"

namespace {

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void bilinear_fwd_kernel(const void* __restrict__ in, int B, int Hi,
                                                           int Wi, int C, int64_t isB, int64_t isH,
                                                           int64_t isW, void* out, int Ho, int Wo,
                                                           int64_t osB, int64_t osH, int64_t osW,
                                                           int accumulate) {
  const int cv = C / 4;
  const int64_t total = (int64_t)B * Ho * Wo * cv;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % cv) * 4;
    int64_t t = i / cv;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    const int64_t base = (int64_t)b * isB + c;
    float a[4], bb[4], cc[4], d[4], o[4];
    if (Hi == Ho && Wi == Wo) {  // identity resize == strided copy / cast / accumulate
      const int64_t ooff = (int64_t)b * osB + (int64_t)oy * osH + (int64_t)ox * osW + c;
      V4<TI>::ld(in, base + oy * isH + ox * isW, a);
      if (accumulate) {
        V4<TO>::ld(out, ooff, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += o[j];
      }
      V4<TO>::st(out, ooff, a);
      continue;
    }
    int y0, y1, x0, x1; float ly, lx;
    src_index2(ry, oy, Hi, y0, y1, ly);
    src_index2(rx, ox, Wi, x0, x1, lx);
    V4<TI>::ld(in, base + y0 * isH + x0 * isW, a);
    V4<TI>::ld(in, base + y0 * isH + x1 * isW, bb);
    V4<TI>::ld(in, base + y1 * isH + x0 * isW, cc);
    V4<TI>::ld(in, base + y1 * isH + x1 * isW, d);
    const int64_t ooff = (int64_t)b * osB + (int64_t)oy * osH + (int64_t)ox * osW + c;
    if (accumulate) V4<TO>::ld(out, ooff, o);
    else { o[0] = o[1] = o[2] = o[3] = 0.f; }
    const float hy = 1.f - ly, hx = 1.f - lx;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] += hy * (hx * a[j] + lx * bb[j]) + ly * (hx * cc[j] + lx * d[j]);
    V4<TO>::st(out, ooff, o);
  }
}

// out = sum_k bilinear(src_k -> Ho x Wo), up to three dense NHWC sources of different sizes with the same channel count,
// ONE write of the output.  Used where a 1x1 convolution over a concat of upsampled pyramid levels is evaluated per
// level at the level's own resolution (a 1x1 convolution and a bilinear resize commute), SegFormer's linear_fuse:
// the upsampled partial results are summed here instead of being written one by one.  Source maps are small (L2-resident).
struct SumSrc { const void* p[3]; int H[3], W[3]; };
// grid = (ceil(Wo * C/VEC / 256), B * Ho): one block per output-row segment, so the batch / row decomposition and every
// source's row pair + vertical weight are block-uniform; a thread only derives its column pair.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void bilinear_sum_kernel(SumSrc src, int nsrc, int B, int C, void* out, int Ho, int Wo) {
  const int cv = C / VEC;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= Wo * cv) return;
  const int ox = j / cv, c = (j - ox * cv) * VEC;
  const int b = blockIdx.y / Ho, oy = blockIdx.y - b * Ho;
  float o[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) o[e] = 0.f;
  for (int k = 0; k < nsrc; ++k) {
    const int Hi = src.H[k], Wi = src.W[k];
    int y0, y1, x0, x1; float ly, lx;
    src_index2((float)Hi / (float)Ho, oy, Hi, y0, y1, ly);
    src_index2((float)Wi / (float)Wo, ox, Wi, x0, x1, lx);
    const int64_t r0 = ((int64_t)b * Hi + y0) * Wi * C + c, r1 = ((int64_t)b * Hi + y1) * Wi * C + c;
    float a[VEC], bb[VEC], cc[VEC], d[VEC];
    if constexpr (VEC == 8) {
      V8::ld(src.p[k], r0 + (int64_t)x0 * C, a);
      V8::ld(src.p[k], r0 + (int64_t)x1 * C, bb);
      V8::ld(src.p[k], r1 + (int64_t)x0 * C, cc);
      V8::ld(src.p[k], r1 + (int64_t)x1 * C, d);
    } else {
      V4<T>::ld(src.p[k], r0 + (int64_t)x0 * C, a);
      V4<T>::ld(src.p[k], r0 + (int64_t)x1 * C, bb);
      V4<T>::ld(src.p[k], r1 + (int64_t)x0 * C, cc);
      V4<T>::ld(src.p[k], r1 + (int64_t)x1 * C, d);
    }
    const float hy = 1.f - ly, hx = 1.f - lx;
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] += hy * (hx * a[e] + lx * bb[e]) + ly * (hx * cc[e] + lx * d[e]);
  }
  const int64_t ooff = (((int64_t)b * Ho + oy) * Wo + ox) * C + c;
  if constexpr (VEC == 8) V8::st(out, ooff, o);
  else V4<T>::st(out, ooff, o);
}

// Strided NHWC copy with dtype conversion (the compute-dtype cast of a channel slice, densifying a strided gradient):
// one thread per (pixel, 4-channel vector); rows of pixels are walked per block so that no 64-bit division runs per element.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void copy_cast_kernel(const void* __restrict__ in, int W, int C, int64_t isB, int64_t isH,
                                                        int64_t isW, void* out, int H, int64_t osB, int64_t osH, int64_t osW) {
  const int cv = C / 4;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= W * cv) return;
  const int x = j / cv, c = (j - x * cv) * 4;
  const int b = blockIdx.y / H, y = blockIdx.y - b * H;
  float v[4];
  V4<TI>::ld(in, (int64_t)b * isB + (int64_t)y * isH + (int64_t)x * isW + c, v);
  V4<TO>::st(out, (int64_t)b * osB + (int64_t)y * osH + (int64_t)x * osW + c, v);
}
// bf16 -> bf16 with 16-byte accesses
__global__ __launch_bounds__(256) void copy8_kernel(const void* __restrict__ in, int W, int C, int64_t isB, int64_t isH,
                                                    int64_t isW, void* out, int H, int64_t osB, int64_t osH, int64_t osW) {
  const int cv = C / 8;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= W * cv) return;
  const int x = j / cv, c = (j - x * cv) * 8;
  const int b = blockIdx.y / H, y = blockIdx.y - b * H;
  const uint4 v = *(const uint4*)((const uint16_t*)in + (int64_t)b * isB + (int64_t)y * isH + (int64_t)x * isW + c);
  *(uint4*)((uint16_t*)out + (int64_t)b * osB + (int64_t)y * osH + (int64_t)x * osW + c) = v;
}

// Backward (gather): din[iy,ix] (+)= sum over outputs whose taps touch (iy,ix).
// Candidate outputs: src in (i-1, i+1)  =>  dst in ((i-0.5)/ratio - 0.5, (i+1.5)/ratio - 0.5).
template <typename TO_, typename TI_>  // TO_ = dtype of dout, TI_ = dtype of din
__global__ __launch_bounds__(256) void bilinear_bwd_kernel(const void* __restrict__ dout, int B, int Ho,
                                                           int Wo, int C, int64_t osB, int64_t osH,
                                                           int64_t osW, void* din, int Hi, int Wi,
                                                           int64_t isB, int64_t isH, int64_t isW,
                                                           int accumulate) {
  const int cv = C / 4;
  const int64_t total = (int64_t)B * Hi * Wi * cv;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % cv) * 4;
    int64_t t = i / cv;
    const int ix = (int)(t % Wi); t /= Wi;
    const int iy = (int)(t % Hi);
    const int b = (int)(t / Hi);
    int oy_lo = (int)floorf(((float)iy - 0.5f) / ry - 0.5f) - 1, oy_hi = (int)ceilf(((float)iy + 1.5f) / ry - 0.5f) + 1;
    int ox_lo = (int)floorf(((float)ix - 0.5f) / rx - 0.5f) - 1, ox_hi = (int)ceilf(((float)ix + 1.5f) / rx - 0.5f) + 1;
    oy_lo = oy_lo < 0 ? 0 : oy_lo; ox_lo = ox_lo < 0 ? 0 : ox_lo;
    oy_hi = oy_hi > Ho - 1 ? Ho - 1 : oy_hi; ox_hi = ox_hi > Wo - 1 ? Wo - 1 : ox_hi;
    float acc[4] = {0, 0, 0, 0};
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      int y0, y1; float ly;
      src_index2(ry, oy, Hi, y0, y1, ly);
      const float wy = (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
      if (wy == 0.f) continue;
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        int x0, x1; float lx;
        src_index2(rx, ox, Wi, x0, x1, lx);
        const float wx = (x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f);
        if (wx == 0.f) continue;
        float g[4];
        V4<TO_>::ld(dout, (int64_t)b * osB + (int64_t)oy * osH + (int64_t)ox * osW + c, g);
        const float w = wy * wx;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += w * g[j];
      }
    }
    const int64_t ioff = (int64_t)b * isB + (int64_t)iy * isH + (int64_t)ix * isW + c;
    if (accumulate) {
      float o[4];
      V4<TI_>::ld(din, ioff, o);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += o[j];
    }
    V4<TI_>::st(din, ioff, acc);
  }
}

// ---- bf16 -> bf16, 8 channels per thread (same arithmetic as the generic kernels above)
__global__ __launch_bounds__(256) void bilinear_fwd8_kernel(const void* __restrict__ in, int B, int Hi, int Wi, int C,
                                                            int64_t isB, int64_t isH, int64_t isW, void* out, int Ho,
                                                            int Wo, int64_t osB, int64_t osH, int64_t osW,
                                                            int accumulate) {
  const int cv = C / 8;
  const int64_t total = (int64_t)B * Ho * Wo * cv;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % cv) * 8;
    int64_t t = i / cv;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    const int64_t base = (int64_t)b * isB + c;
    const int64_t ooff = (int64_t)b * osB + (int64_t)oy * osH + (int64_t)ox * osW + c;
    float a[8], bb[8], cc[8], d[8], o[8];
    if (Hi == Ho && Wi == Wo) {
      V8::ld(in, base + oy * isH + ox * isW, a);
      if (accumulate) {
        V8::ld(out, ooff, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += o[j];
      }
      V8::st(out, ooff, a);
      continue;
    }
    int y0, y1, x0, x1; float ly, lx;
    src_index2(ry, oy, Hi, y0, y1, ly);
    src_index2(rx, ox, Wi, x0, x1, lx);
    V8::ld(in, base + y0 * isH + x0 * isW, a);
    V8::ld(in, base + y0 * isH + x1 * isW, bb);
    V8::ld(in, base + y1 * isH + x0 * isW, cc);
    V8::ld(in, base + y1 * isH + x1 * isW, d);
    if (accumulate) V8::ld(out, ooff, o);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = 0.f;
    }
    const float hy = 1.f - ly, hx = 1.f - lx;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] += hy * (hx * a[j] + lx * bb[j]) + ly * (hx * cc[j] + lx * d[j]);
    V8::st(out, ooff, o);
  }
}

__global__ __launch_bounds__(256) void bilinear_bwd8_kernel(const void* __restrict__ dout, int B, int Ho, int Wo, int C,
                                                            int64_t osB, int64_t osH, int64_t osW, void* din, int Hi,
                                                            int Wi, int64_t isB, int64_t isH, int64_t isW,
                                                            int accumulate) {
  const int cv = C / 8;
  const int64_t total = (int64_t)B * Hi * Wi * cv;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % cv) * 8;
    int64_t t = i / cv;
    const int ix = (int)(t % Wi); t /= Wi;
    const int iy = (int)(t % Hi);
    const int b = (int)(t / Hi);
    int oy_lo = (int)floorf(((float)iy - 0.5f) / ry - 0.5f) - 1, oy_hi = (int)ceilf(((float)iy + 1.5f) / ry - 0.5f) + 1;
    int ox_lo = (int)floorf(((float)ix - 0.5f) / rx - 0.5f) - 1, ox_hi = (int)ceilf(((float)ix + 1.5f) / rx - 0.5f) + 1;
    oy_lo = oy_lo < 0 ? 0 : oy_lo; ox_lo = ox_lo < 0 ? 0 : ox_lo;
    oy_hi = oy_hi > Ho - 1 ? Ho - 1 : oy_hi; ox_hi = ox_hi > Wo - 1 ? Wo - 1 : ox_hi;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      int y0, y1; float ly;
      src_index2(ry, oy, Hi, y0, y1, ly);
      const float wy = (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
      if (wy == 0.f) continue;
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        int x0, x1; float lx;
        src_index2(rx, ox, Wi, x0, x1, lx);
        const float wx = (x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f);
        if (wx == 0.f) continue;
        float g[8];
        V8::ld(dout, (int64_t)b * osB + (int64_t)oy * osH + (int64_t)ox * osW + c, g);
        const float w = wy * wx;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += w * g[j];
      }
    }
    const int64_t ioff = (int64_t)b * isB + (int64_t)iy * isH + (int64_t)ix * isW + c;
    if (accumulate) {
      float o[8];
      V8::ld(din, ioff, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += o[j];
    }
    V8::st(din, ioff, acc);
  }
}

// Large upsampling factors (UperNet's pyramid pooling: 1x1 .. 6x6 maps resized to 18 x 18, factors 3 .. 18): an input pixel
// gathers from up to (2 f + 2)^2 output pixels, and the flat kernel above walks that window with ONE thread per 8 channels --
// 324 dependent 16-byte loads for the 1x1 branch, 1024 threads on the whole chip: 112 us at batch 4, 162 us at batch 32.
// Here a block owns one input pixel: 32 lanes cover 256 channels, the 8 lane groups split the window rows, LDS adds the
// eight partial sums in a fixed order.
__global__ __launch_bounds__(256) void bilinear_bwd8_window_kernel(const void* __restrict__ dout, int Ho, int Wo, int C,
                                                                   int64_t osB, int64_t osH, int64_t osW, void* din, int Hi,
                                                                   int Wi, int64_t isB, int64_t isH, int64_t isW, int accumulate) {
  __shared__ float red[8][32][8];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int c = (blockIdx.x * 32 + cl) * 8;
  int t = blockIdx.y;
  const int ix = t % Wi; t /= Wi;
  const int iy = t % Hi;
  const int b = t / Hi;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  int oy_lo = (int)floorf(((float)iy - 0.5f) / ry - 0.5f) - 1, oy_hi = (int)ceilf(((float)iy + 1.5f) / ry - 0.5f) + 1;
  int ox_lo = (int)floorf(((float)ix - 0.5f) / rx - 0.5f) - 1, ox_hi = (int)ceilf(((float)ix + 1.5f) / rx - 0.5f) + 1;
  oy_lo = oy_lo < 0 ? 0 : oy_lo; ox_lo = ox_lo < 0 ? 0 : ox_lo;
  oy_hi = oy_hi > Ho - 1 ? Ho - 1 : oy_hi; ox_hi = ox_hi > Wo - 1 ? Wo - 1 : ox_hi;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (c < C) {
    for (int oy = oy_lo + sl; oy <= oy_hi; oy += 8) {
      int y0, y1; float ly;
      src_index2(ry, oy, Hi, y0, y1, ly);
      const float wy = (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
      if (wy == 0.f) continue;
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        int x0, x1; float lx;
        src_index2(rx, ox, Wi, x0, x1, lx);
        const float wx = (x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f);
        if (wx == 0.f) continue;
        float g[8];
        V8::ld(dout, (int64_t)b * osB + (int64_t)oy * osH + (int64_t)ox * osW + c, g);
        const float w = wy * wx;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += w * g[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[sl][cl][j] = acc[j];
  __syncthreads();
  if (sl != 0 || c >= C) return;
#pragma unroll
  for (int k = 1; k < 8; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += red[k][cl][j];
  const int64_t ioff = (int64_t)b * isB + (int64_t)iy * isH + (int64_t)ix * isW + c;
  if (accumulate) {
    float o[8];
    V8::ld(din, ioff, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += o[j];
  }
  V8::st(din, ioff, acc);
}

// ---- row-structured versions of the two 8-channel kernels: blockIdx.y = (batch, row), so the row decomposition and the
// vertical source index are per-block scalars and a thread divides once (the flat kernels above spend ~100 VALU
// instructions of index arithmetic per 16 bytes and ran at 2.3 TB/s; DOFA's resamples are 5.6 % of the train step).
// Same arithmetic, same summation order -> bit-identical results.
__global__ __launch_bounds__(256) void bilinear_fwd8_rows_kernel(const void* __restrict__ in, int Hi, int Wi, int C,
                                                                 int64_t isB, int64_t isH, int64_t isW, void* out,
                                                                 int Ho, int Wo, int64_t osB, int64_t osH, int64_t osW,
                                                                 int accumulate) {
  const int cv = C / 8;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= Wo * cv) return;
  const int b = blockIdx.y / Ho, oy = blockIdx.y - b * Ho;
  const int ox = j / cv, c = (j - ox * cv) * 8;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  const int64_t base = (int64_t)b * isB + c;
  const int64_t ooff = (int64_t)b * osB + (int64_t)oy * osH + (int64_t)ox * osW + c;
  float a[8], bb[8], cc[8], d[8], o[8];
  if (Hi == Ho && Wi == Wo) {
    V8::ld(in, base + oy * isH + ox * isW, a);
    if (accumulate) {
      V8::ld(out, ooff, o);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += o[e];
    }
    V8::st(out, ooff, a);
    return;
  }
  int y0, y1, x0, x1; float ly, lx;
  src_index2(ry, oy, Hi, y0, y1, ly);
  src_index2(rx, ox, Wi, x0, x1, lx);
  V8::ld(in, base + y0 * isH + x0 * isW, a);
  V8::ld(in, base + y0 * isH + x1 * isW, bb);
  V8::ld(in, base + y1 * isH + x0 * isW, cc);
  V8::ld(in, base + y1 * isH + x1 * isW, d);
  if (accumulate) V8::ld(out, ooff, o);
  else {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
  }
  const float hy = 1.f - ly, hx = 1.f - lx;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] += hy * (hx * a[e] + lx * bb[e]) + ly * (hx * cc[e] + lx * d[e]);
  V8::st(out, ooff, o);
}

// Exact integer upsampling factors (F = 2, 4: the FPN top-down path, the pyramid levels of fpn_bottleneck's concat): a thread owns
// the GAP between four neighbouring input pixels -- the F x F output pixels whose two source rows and two source columns are
// those four -- loads them once and writes F x F outputs (the row kernel above loads four 16-byte pieces per 16 bytes stored:
// 2.65 TB/s on a write-bound op).  Gaps -1 and Hi - 1 (Wi - 1) are the clamped borders with F / 2 rows (columns).  Same
// source indices, weights and expression per output as bilinear_fwd8_rows_kernel: bit-identical results.
// BN (the top-down add of a TRAINING lateral): acc_src is the lateral's PRE-BatchNorm convolution output and every vector read from
// it becomes bf16(relu?((x - mean) * (rstd gamma) + beta)) first -- bn_apply_kernel's f32 expression and its one bf16 rounding
// (norm.hip), so the sum is bit for bit what bn_apply followed by this kernel gives and the normalised lateral is never written.
// A thread's channels are fixed: 24 constants in registers.
template <int F, bool BN>
__global__ __launch_bounds__(256) void bilinear_fwd8_gap_kernel(const void* __restrict__ in, int Hi, int Wi, int C,
                                                                int64_t isB, int64_t isH, int64_t isW, void* out,
                                                                int64_t osB, int64_t osH, int64_t osW, const void* acc_src,
                                                                const float* __restrict__ mean, const float* __restrict__ var,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float eps, int relu) {
  // acc_src: nullptr, `out` itself (out += result) or another map with out's strides (out = that + result: the FPN top-down add
  // without first copying the lateral into the output)
  const int cv = C / 8;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= (Wi + 1) * cv) return;
  const int Ho = F * Hi, Wo = F * Wi;
  const int b = blockIdx.y / (Hi + 1), gy = blockIdx.y - b * (Hi + 1);     // gap gy: output rows F gy - F/2 .. F gy + F/2 - 1
  const int gx = j / cv, c = (j - gx * cv) * 8;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  const int oy0 = F * gy - F / 2 < 0 ? 0 : F * gy - F / 2, ox0 = F * gx - F / 2 < 0 ? 0 : F * gx - F / 2;
  int y0, y1, x0, x1; float l;
  src_index2(ry, oy0, Hi, y0, y1, l);
  src_index2(rx, ox0, Wi, x0, x1, l);
  const int64_t base = (int64_t)b * isB + c;
  float a[8], bb[8], cc[8], d[8];
  V8::ld(in, base + y0 * isH + x0 * isW, a);
  V8::ld(in, base + y0 * isH + x1 * isW, bb);
  V8::ld(in, base + y1 * isH + x0 * isW, cc);
  V8::ld(in, base + y1 * isH + x1 * isW, d);
  float mu[BN ? 8 : 1], sc[BN ? 8 : 1], be[BN ? 8 : 1];
  if constexpr (BN) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { mu[e] = mean[c + e]; sc[e] = rsqrtf(var[c + e] + eps) * gamma[c + e]; be[e] = beta[c + e]; }
  }
#pragma unroll
  for (int jy = 0; jy < F; ++jy) {
    const int oy = F * gy - F / 2 + jy;
    if (oy < 0 || oy >= Ho) continue;
    int t0, t1; float ly;
    src_index2(ry, oy, Hi, t0, t1, ly);
    const float hy = 1.f - ly;
#pragma unroll
    for (int jx = 0; jx < F; ++jx) {
      const int ox = F * gx - F / 2 + jx;
      if (ox < 0 || ox >= Wo) continue;
      float lx;
      src_index2(rx, ox, Wi, t0, t1, lx);
      const float hx = 1.f - lx;
      const int64_t ooff = (int64_t)b * osB + (int64_t)oy * osH + (int64_t)ox * osW + c;
      float o[8];
      if (acc_src) V8::ld(acc_src, ooff, o);
      else {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = 0.f;
      }
      if constexpr (BN) {
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          const float u = (o[e] - mu[e]) * sc[e] + be[e], v = (o[e + 1] - mu[e + 1]) * sc[e + 1] + be[e + 1];
          const uint32_t z = pack_bf16x2(relu ? fmaxf(u, 0.f) : u, relu ? fmaxf(v, 0.f) : v);
          o[e] = __uint_as_float(z << 16); o[e + 1] = __uint_as_float(z & 0xffff0000u);
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] += hy * (hx * a[e] + lx * bb[e]) + ly * (hx * cc[e] + lx * d[e]);
      V8::st(out, ooff, o);
    }
  }
}

// NX = upper bound of the horizontal output window of one input pixel (2 * ceil(Wo / Wi) + 4); the window's weights are
// computed once per thread instead of once per (output row, output column)
template <int NX>
__global__ __launch_bounds__(256) void bilinear_bwd8_rows_kernel(const void* __restrict__ dout, int Ho, int Wo, int C,
                                                                 int64_t osB, int64_t osH, int64_t osW, void* din,
                                                                 int Hi, int Wi, int64_t isB, int64_t isH, int64_t isW,
                                                                 int accumulate) {
  const int cv = C / 8;
  // Neighbouring input rows gather from overlapping dout rows (a x4 resize: 8 dout rows per input row, 4 apart).  Dealt
  // out in launch order, consecutive blocks land on different XCDs and every L2 fetches its own copy (PMC: 1.30 GB fetched
  // per launch for 0.34 GB of dout); with the XCD-major order one XCD walks a contiguous band of rows.
  const int nblk = gridDim.x * gridDim.y;
  const int id = blockIdx.y * gridDim.x + blockIdx.x;
  const int q8 = nblk >> 3, r8 = nblk & 7, xcd = id & 7, idx = id >> 3;
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  const int brow = lid / gridDim.x, bx = lid - brow * gridDim.x;
  const int j = bx * 256 + threadIdx.x;
  if (j >= Wi * cv) return;
  const int b = brow / Hi, iy = brow - b * Hi;
  const int ix = j / cv, c = (j - ix * cv) * 8;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  int oy_lo = (int)floorf(((float)iy - 0.5f) / ry - 0.5f) - 1, oy_hi = (int)ceilf(((float)iy + 1.5f) / ry - 0.5f) + 1;
  int ox_lo = (int)floorf(((float)ix - 0.5f) / rx - 0.5f) - 1, ox_hi = (int)ceilf(((float)ix + 1.5f) / rx - 0.5f) + 1;
  oy_lo = oy_lo < 0 ? 0 : oy_lo; ox_lo = ox_lo < 0 ? 0 : ox_lo;
  oy_hi = oy_hi > Ho - 1 ? Ho - 1 : oy_hi; ox_hi = ox_hi > Wo - 1 ? Wo - 1 : ox_hi;
  float wx[NX];
#pragma unroll
  for (int k = 0; k < NX; ++k) {
    const int ox = ox_lo + k;
    wx[k] = 0.f;
    if (ox <= ox_hi) {
      int x0, x1; float lx;
      src_index2(rx, ox, Wi, x0, x1, lx);
      wx[k] = (x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f);
    }
  }
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  const int64_t col = (int64_t)b * osB + (int64_t)ox_lo * osW + c;
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {
    int y0, y1; float ly;
    src_index2(ry, oy, Hi, y0, y1, ly);
    const float wy = (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
    if (wy == 0.f) continue;                               // uniform over the block
    const int64_t rowoff = col + (int64_t)oy * osH;
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      if (wx[k] == 0.f) continue;
      float g[8];
      V8::ld(dout, rowoff + (int64_t)k * osW, g);
      const float w = wy * wx[k];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += w * g[e];
    }
  }
  const int64_t ioff = (int64_t)b * isB + (int64_t)iy * isH + (int64_t)ix * isW + c;
  if (accumulate) {
    float o[8];
    V8::ld(din, ioff, o);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += o[e];
  }
  V8::st(din, ioff, acc);
}

// Exact integer factors (F = 2, 4): a thread WALKS DOWN a column of input pixels.  The F gradient rows between input rows g - 1
// and g feed both of them (weights 1 - ly and ly): they are loaded once and added to two running accumulators, instead of once
// per input row (the row kernel above fetches 4 F^2 pieces per input pixel, this one 2 F^2 (1 + 1 / RSEG)).  A block column is cut
// into segments of RSEG input rows for parallelism; the gap rows on a segment border are read by both neighbours.  Every input
// pixel receives its terms in the row kernel's order (gradient rows ascending, window columns ascending, zero weights skipped)
// with the same products: bit-identical results.
template <int F, int RSEG>
__global__ __launch_bounds__(256) void bilinear_bwd8_walk_kernel(const void* __restrict__ dout, int C, int64_t osB, int64_t osH,
                                                                 int64_t osW, void* din, int Hi, int Wi, int64_t isB, int64_t isH,
                                                                 int64_t isW, int accumulate) {
  const int cv = C / 8, Ho = F * Hi, Wo = F * Wi;
  // XCD-major block order (as in the row kernel): horizontally neighbouring blocks read overlapping gradient columns (a window
  // of 2 F columns every F) and vertically neighbouring segments share their border rows -- one XCD walks a contiguous range
  const int nblk = gridDim.x * gridDim.y;
  const int id = blockIdx.y * gridDim.x + blockIdx.x;
  const int q8 = nblk >> 3, r8 = nblk & 7, xcd = id & 7, idx = id >> 3;
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  const int brow = lid / gridDim.x, bx = lid - brow * gridDim.x;
  const int j = bx * 256 + threadIdx.x;
  if (j >= Wi * cv) return;
  const int nseg = (Hi + RSEG - 1) / RSEG;
  const int b = brow / nseg, seg = brow - b * nseg;
  const int iy0 = seg * RSEG, iy1 = iy0 + RSEG < Hi ? iy0 + RSEG : Hi;
  const int ix = j / cv, c = (j - ix * cv) * 8;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  // the window columns with a non-zero weight are exactly F ix - F/2 .. F ix + 3F/2 - 1 (inside the image); a column outside is
  // fetched from the clamped address -- UNCONDITIONAL loads, so that the 2 F pieces of a gradient row are in flight together
  // (inside `if (wx[k] == 0.f) continue` every load waited for its predecessor's multiply-adds) -- and its term is not added
  constexpr int NW = 2 * F;
  float wx[NW];
  int64_t coff[NW];
  unsigned okmask = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const int ox = F * ix - F / 2 + k;
    const bool ok = ox >= 0 && ox < Wo;
    const int oxc = ox < 0 ? 0 : (ox > Wo - 1 ? Wo - 1 : ox);
    int x0, x1; float lx;
    src_index2(rx, oxc, Wi, x0, x1, lx);
    wx[k] = (x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f);
    coff[k] = (int64_t)oxc * osW;
    okmask |= (ok ? 1u : 0u) << k;
  }
  const int64_t col = (int64_t)b * osB + c;
  float up[8], dn[8];        // accumulators of input rows g - 1 and g while gap g is walked
#pragma unroll
  for (int e = 0; e < 8; ++e) up[e] = dn[e] = 0.f;
  for (int g = iy0; g <= iy1; ++g) {                       // gap g: gradient rows F g - F/2 .. F g + F/2 - 1 (source rows g - 1, g)
#pragma unroll
    for (int jy = 0; jy < F; ++jy) {
      const int oy = F * g - F / 2 + jy;
      if (oy < 0 || oy >= Ho) continue;                    // (uniform)
      int y0, y1; float ly;
      src_index2(ry, oy, Hi, y0, y1, ly);
      // weights of this gradient row for input rows g - 1 and g, as the row kernel forms them for each of the two
      const float w_up = g - 1 >= iy0 ? (y0 == g - 1 ? 1.f - ly : 0.f) + (y1 == g - 1 ? ly : 0.f) : 0.f;
      const float w_dn = g < iy1 ? (y0 == g ? 1.f - ly : 0.f) + (y1 == g ? ly : 0.f) : 0.f;
      if (w_up == 0.f && w_dn == 0.f) continue;            // (uniform)
      const int64_t rowoff = col + (int64_t)oy * osH;
      float v[NW][8];
#pragma unroll
      for (int k = 0; k < NW; ++k) V8::ld(dout, rowoff + coff[k], v[k]);
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        const bool ok = (okmask >> k) & 1u;
        if (w_up != 0.f) {                                 // (uniform)
          const float w = w_up * wx[k];
#pragma unroll
          for (int e = 0; e < 8; ++e) up[e] = ok ? up[e] + w * v[k][e] : up[e];
        }
        if (w_dn != 0.f) {
          const float w = w_dn * wx[k];
#pragma unroll
          for (int e = 0; e < 8; ++e) dn[e] = ok ? dn[e] + w * v[k][e] : dn[e];
        }
      }
    }
    if (g - 1 >= iy0) {                                    // input row g - 1 is complete
      const int64_t ioff = (int64_t)b * isB + (int64_t)(g - 1) * isH + (int64_t)ix * isW + c;
      if (accumulate) {
        float o[8];
        V8::ld(din, ioff, o);
#pragma unroll
        for (int e = 0; e < 8; ++e) up[e] += o[e];
      }
      V8::st(din, ioff, up);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { up[e] = dn[e]; dn[e] = 0.f; }
  }
}

// nn.AdaptiveAvgPool2d: bin i covers [floor(i*In/S), ceil((i+1)*In/S))
__device__ __forceinline__ void pool_bin(int i, int in, int s, int& lo, int& hi) {
  lo = (i * in) / s;
  hi = ((i + 1) * in + s - 1) / s;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const void* __restrict__ in, int B, int Hi, int Wi,
                                                          int C, int64_t isB, int64_t isH, int64_t isW,
                                                          void* out, int S) {
  const int cv = C / 4;
  const int64_t total = (int64_t)B * S * S * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % cv) * 4;
    int64_t t = i / cv;
    const int ox = (int)(t % S); t /= S;
    const int oy = (int)(t % S);
    const int b = (int)(t / S);
    int y0, y1, x0, x1;
    pool_bin(oy, Hi, S, y0, y1);
    pool_bin(ox, Wi, S, x0, x1);
    float acc[4] = {0, 0, 0, 0};
    for (int y = y0; y < y1; ++y)
      for (int x = x0; x < x1; ++x) {
        float v[4];
        V4<TI>::ld(in, (int64_t)b * isB + y * isH + x * isW + c, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += v[j];
      }
    const float inv = 1.f / (float)((y1 - y0) * (x1 - x0));
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] *= inv;
    V4<TO>::st(out, (((int64_t)b * S + oy) * S + ox) * C + c, acc);
  }
}

// Large bins (pyramid pooling of an 18 x 18 map into 1 .. 3 bins per side: 36 .. 324 pixels each): the kernel above sums a bin
// with one thread per 4 channels -- 35 us whatever the batch.  Here 32 lanes cover 128 channels and the block's 8 lane groups
// split the bin's rows; LDS adds the partial sums in a fixed order.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void avgpool_fwd_split_kernel(const void* __restrict__ in, int Hi, int Wi, int C, int64_t isB,
                                                                int64_t isH, int64_t isW, void* out, int S) {
  __shared__ float red[8][32][4];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int c = (blockIdx.x * 32 + cl) * 4;
  int t = blockIdx.y;
  const int ox = t % S; t /= S;
  const int oy = t % S;
  const int b = t / S;
  int y0, y1, x0, x1;
  pool_bin(oy, Hi, S, y0, y1);
  pool_bin(ox, Wi, S, x0, x1);
  float acc[4] = {0, 0, 0, 0};
  if (c < C) {
    for (int y = y0 + sl; y < y1; y += 8)
      for (int x = x0; x < x1; ++x) {
        float v[4];
        V4<TI>::ld(in, (int64_t)b * isB + y * isH + x * isW + c, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += v[j];
      }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[sl][cl][j] = acc[j];
  __syncthreads();
  if (sl != 0 || c >= C) return;
#pragma unroll
  for (int k = 1; k < 8; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += red[k][cl][j];
  const float inv = 1.f / (float)((y1 - y0) * (x1 - x0));
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] *= inv;
  V4<TO>::st(out, (((int64_t)b * S + oy) * S + ox) * C + c, acc);
}

template <typename TO_, typename TI_>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const void* __restrict__ dout, int B, int S, int C,
                                                          void* din, int Hi, int Wi, int64_t isB,
                                                          int64_t isH, int64_t isW, int accumulate) {
  const int cv = C / 4;
  const int64_t total = (int64_t)B * Hi * Wi * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % cv) * 4;
    int64_t t = i / cv;
    const int x = (int)(t % Wi); t /= Wi;
    const int y = (int)(t % Hi);
    const int b = (int)(t / Hi);
    float acc[4] = {0, 0, 0, 0};
    for (int oy = 0; oy < S; ++oy) {
      int y0, y1;
      pool_bin(oy, Hi, S, y0, y1);
      if (y < y0 || y >= y1) continue;
      for (int ox = 0; ox < S; ++ox) {
        int x0, x1;
        pool_bin(ox, Wi, S, x0, x1);
        if (x < x0 || x >= x1) continue;
        float g[4];
        V4<TO_>::ld(dout, (((int64_t)b * S + oy) * S + ox) * C + c, g);
        const float inv = 1.f / (float)((y1 - y0) * (x1 - x0));
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += g[j] * inv;
      }
    }
    const int64_t ioff = (int64_t)b * isB + (int64_t)y * isH + (int64_t)x * isW + c;
    if (accumulate) {
      float o[4];
      V4<TI_>::ld(din, ioff, o);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += o[j];
    }
    V4<TI_>::st(din, ioff, acc);
  }
}

inline unsigned resample_grid_for(int64_t total) {
  int64_t g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

#define DISPATCH2(KERN, DA, DB, ...)                                                                 \
  do {                                                                                               \
    if ((DA) == GDL_BF16 && (DB) == GDL_BF16) hipLaunchKernelGGL((KERN<uint16_t, uint16_t>), __VA_ARGS__); \
    else if ((DA) == GDL_BF16) hipLaunchKernelGGL((KERN<uint16_t, float>), __VA_ARGS__);             \
    else if ((DB) == GDL_BF16) hipLaunchKernelGGL((KERN<float, uint16_t>), __VA_ARGS__);             \
    else hipLaunchKernelGGL((KERN<float, float>), __VA_ARGS__);                                      \
  } while (0)

int g_flat_resample = 0;   // A/B hook: 1 = the flat-index kernels

inline bool vec8_ok(const void* a, const void* b, int C, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                    int64_t s5) {
  return C % 8 == 0 && ((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0) && s0 % 8 == 0 && s1 % 8 == 0 &&
         s2 % 8 == 0 && s3 % 8 == 0 && s4 % 8 == 0 && s5 % 8 == 0;
}

// the exact integer factor of an upsampling (the same in both directions, from a map of more than one row and column), else 0
inline int integer_factor(int Hi, int Wi, int Ho, int Wo) {
  return (Hi > 1 && Wi > 1 && Ho % Hi == 0 && Wo % Wi == 0 && Ho / Hi == Wo / Wi) ? Ho / Hi : 0;
}

}  // namespace

extern "C" void gdl_debug_set_flat_resample(int on) { g_flat_resample = on; }

static int bilinear_fwd_impl(const void* in, int in_dtype, int B, int Hi, int Wi, int C, int64_t isB,
                             int64_t isH, int64_t isW, void* out, int out_dtype, int Ho, int Wo,
                             int64_t osB, int64_t osH, int64_t osW, int accumulate, const void* base,
                             gdl_stream_t stream) {
  GDL_CHECK_ARG(in && out, "gdl_bilinear_fwd: null pointer");
  GDL_CHECK_ARG(C % 4 == 0 && isB % 4 == 0 && isH % 4 == 0 && isW % 4 == 0 && osB % 4 == 0 && osH % 4 == 0 &&
                    osW % 4 == 0, "gdl_bilinear_fwd: C and strides must be multiples of 4");
  if (in_dtype == GDL_BF16 && out_dtype == GDL_BF16 && vec8_ok(in, out, C, isB, isH, isW, osB, osH, osW)) {
    const int64_t total8 = (int64_t)B * Ho * Wo * (C / 8);
    const int fac = integer_factor(Hi, Wi, Ho, Wo);
    const bool gap = (fac == 2 || fac == 4) && (int64_t)B * (Hi + 1) <= 65535 && !g_flat_resample;
    if (base && !(gap && (uintptr_t)base % 16 == 0)) return GDL_ERR_UNSUPPORTED;      // (the caller copies + accumulates)
    if (gap) {
      const dim3 grid((unsigned)(((Wi + 1) * (C / 8) + 255) / 256), (unsigned)(B * (Hi + 1)));
      const void* acc_src = base ? base : (accumulate ? out : nullptr);
      const float* none = nullptr;
      if (fac == 2) hipLaunchKernelGGL((bilinear_fwd8_gap_kernel<2, false>), grid, dim3(256), 0, (hipStream_t)stream, in, Hi, Wi, C, isB, isH, isW, out, osB, osH, osW, acc_src, none, none, none, none, 0.f, 0);
      else hipLaunchKernelGGL((bilinear_fwd8_gap_kernel<4, false>), grid, dim3(256), 0, (hipStream_t)stream, in, Hi, Wi, C, isB, isH, isW, out, osB, osH, osW, acc_src, none, none, none, none, 0.f, 0);
    } else if ((int64_t)B * Ho <= 65535 && g_flat_resample != 1)
      hipLaunchKernelGGL(bilinear_fwd8_rows_kernel, dim3((unsigned)((Wo * (C / 8) + 255) / 256), (unsigned)(B * Ho)), dim3(256), 0,
                         (hipStream_t)stream, in, Hi, Wi, C, isB, isH, isW, out, Ho, Wo, osB, osH, osW, accumulate);
    else
    hipLaunchKernelGGL(bilinear_fwd8_kernel, dim3(resample_grid_for(total8)), dim3(256), 0, (hipStream_t)stream, in, B, Hi, Wi, C,
                       isB, isH, isW, out, Ho, Wo, osB, osH, osW, accumulate);
    GDL_CHECK_LAUNCH("gdl_bilinear_fwd");
    return GDL_OK;
  }
  if (base) return GDL_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)B * Ho * Wo * (C / 4);
  DISPATCH2(bilinear_fwd_kernel, in_dtype, out_dtype, dim3(resample_grid_for(total)), dim3(256), 0,
            (hipStream_t)stream, in, B, Hi, Wi, C, isB, isH, isW, out, Ho, Wo, osB, osH, osW, accumulate);
  GDL_CHECK_LAUNCH("gdl_bilinear_fwd");
  return GDL_OK;
}

extern "C" int gdl_bilinear_fwd(const void* in, int in_dtype, int B, int Hi, int Wi, int C, int64_t isB,
                                int64_t isH, int64_t isW, void* out, int out_dtype, int Ho, int Wo,
                                int64_t osB, int64_t osH, int64_t osW, int accumulate,
                                gdl_stream_t stream) {
  return bilinear_fwd_impl(in, in_dtype, B, Hi, Wi, C, isB, isH, isW, out, out_dtype, Ho, Wo, osB, osH, osW, accumulate, nullptr, stream);
}

extern "C" int gdl_bilinear_fwd_add(const void* in, int in_dtype, int B, int Hi, int Wi, int C, int64_t isB,
                                    int64_t isH, int64_t isW, const void* base, void* out, int out_dtype, int Ho, int Wo,
                                    int64_t osB, int64_t osH, int64_t osW, gdl_stream_t stream) {
  GDL_CHECK_ARG(in && base && out, "gdl_bilinear_fwd_add: null pointer");
  // one pass where the gap kernel applies (bf16, 16-byte vectors, factor 2 / 4); otherwise the lateral is copied and the resized
  // map accumulated into it -- same values either way (out = base, then += the interpolation in f32, rounded once)
  const int st = bilinear_fwd_impl(in, in_dtype, B, Hi, Wi, C, isB, isH, isW, out, out_dtype, Ho, Wo, osB, osH, osW, 0, base, stream);
  if (st != GDL_ERR_UNSUPPORTED) return st;
  const int st2 = gdl_copy_cast(base, out_dtype, B, Ho, Wo, C, osB, osH, osW, out, out_dtype, osB, osH, osW, stream);
  if (st2 != GDL_OK) return st2;
  return bilinear_fwd_impl(in, in_dtype, B, Hi, Wi, C, isB, isH, isW, out, out_dtype, Ho, Wo, osB, osH, osW, 1, nullptr, stream);
}

// gdl_bilinear_fwd_add with base = relu?(bn(x)) formed on the fly from the pre-BatchNorm map x [B, Ho, Wo, C] (dense) and the
// per-channel statistics / affine parameters: the top-down add of a training lateral without the bn_apply pass.  Only the one-pass
// gap kernel has this form (dense 16-byte aligned bf16, C % 8 == 0, factor 2 or 4: gdl_bilinear_fwd_add_bn_ok); there is no copy +
// accumulate fallback -- other shapes fail and the caller runs gdl_bn_apply + gdl_bilinear_fwd_add.
extern "C" int gdl_bilinear_fwd_add_bn_ok(int dtype, int B, int Hi, int Wi, int Ho, int Wo, int C) {
  const int fac = integer_factor(Hi, Wi, Ho, Wo);
  return dtype == GDL_BF16 && B > 0 && C > 0 && C % 8 == 0 && (fac == 2 || fac == 4) && (int64_t)B * (Hi + 1) <= 65535 && !g_flat_resample;
}

extern "C" int gdl_bilinear_fwd_add_bn(const void* in, int dtype, int B, int Hi, int Wi, int C, const void* x, const float* mean,
                                       const float* var, const float* gamma, const float* beta, float eps, int relu, void* out,
                                       int Ho, int Wo, gdl_stream_t stream) {
  GDL_CHECK_ARG(in && x && mean && var && gamma && beta && out, "gdl_bilinear_fwd_add_bn: null pointer");
  GDL_CHECK_ARG(gdl_bilinear_fwd_add_bn_ok(dtype, B, Hi, Wi, Ho, Wo, C) && (uintptr_t)in % 16 == 0 && (uintptr_t)x % 16 == 0 &&
                    (uintptr_t)out % 16 == 0,
                "gdl_bilinear_fwd_add_bn: needs dense 16-byte aligned bf16 maps, C %% 8 == 0 and a resize factor of 2 or 4");
  const int64_t isW = C, isH = (int64_t)Wi * C, isB = (int64_t)Hi * isH, osW = C, osH = (int64_t)Wo * C, osB = (int64_t)Ho * osH;
  const dim3 grid((unsigned)(((Wi + 1) * (C / 8) + 255) / 256), (unsigned)(B * (Hi + 1)));
  if (Ho / Hi == 2) hipLaunchKernelGGL((bilinear_fwd8_gap_kernel<2, true>), grid, dim3(256), 0, (hipStream_t)stream, in, Hi, Wi, C, isB, isH, isW, out, osB, osH, osW, x, mean, var, gamma, beta, eps, relu);
  else hipLaunchKernelGGL((bilinear_fwd8_gap_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)stream, in, Hi, Wi, C, isB, isH, isW, out, osB, osH, osW, x, mean, var, gamma, beta, eps, relu);
  GDL_CHECK_LAUNCH("gdl_bilinear_fwd_add_bn");
  return GDL_OK;
}

extern "C" int gdl_copy_cast(const void* in, int in_dtype, int B, int H, int W, int C, int64_t isB, int64_t isH, int64_t isW,
                             void* out, int out_dtype, int64_t osB, int64_t osH, int64_t osW, gdl_stream_t stream) {
  GDL_CHECK_ARG(in && out && B > 0 && H > 0 && W > 0 && C > 0, "gdl_copy_cast: bad args");
  GDL_CHECK_ARG((in_dtype == GDL_F32 || in_dtype == GDL_BF16) && (out_dtype == GDL_F32 || out_dtype == GDL_BF16), "gdl_copy_cast: bad dtype");
  GDL_CHECK_ARG(C % 4 == 0 && isB % 4 == 0 && isH % 4 == 0 && isW % 4 == 0 && osB % 4 == 0 && osH % 4 == 0 && osW % 4 == 0 &&
                    (uintptr_t)in % 8 == 0 && (uintptr_t)out % 8 == 0,
                "gdl_copy_cast: C, strides and pointers must keep 4-channel alignment");
  GDL_CHECK_ARG((int64_t)B * H <= 65535 * 1ll, "gdl_copy_cast: B * H must fit one grid dimension");
  if (in_dtype == GDL_BF16 && out_dtype == GDL_BF16 && vec8_ok(in, out, C, isB, isH, isW, osB, osH, osW)) {
    hipLaunchKernelGGL(copy8_kernel, dim3((unsigned)((W * (C / 8) + 255) / 256), (unsigned)(B * H)), dim3(256), 0,
                       (hipStream_t)stream, in, W, C, isB, isH, isW, out, H, osB, osH, osW);
  } else {
    const dim3 grid((unsigned)((W * (C / 4) + 255) / 256), (unsigned)(B * H));
    DISPATCH2(copy_cast_kernel, in_dtype, out_dtype, grid, dim3(256), 0, (hipStream_t)stream, in, W, C, isB, isH, isW, out, H, osB,
              osH, osW);
  }
  GDL_CHECK_LAUNCH("gdl_copy_cast");
  return GDL_OK;
}

extern "C" int gdl_bilinear_sum_fwd(const void* const* srcs, const int* hs, const int* ws, int nsrc, int dtype, int B, int C,
                                    void* out, int Ho, int Wo, gdl_stream_t stream) {
  GDL_CHECK_ARG(srcs && hs && ws && out && nsrc >= 1 && nsrc <= 3, "gdl_bilinear_sum_fwd: 1..3 sources");
  GDL_CHECK_ARG(dtype == GDL_F32 || dtype == GDL_BF16, "gdl_bilinear_sum_fwd: bad dtype");
  GDL_CHECK_ARG(B > 0 && Ho > 0 && Wo > 0 && C > 0 && C % (dtype == GDL_BF16 ? 8 : 4) == 0,
                "gdl_bilinear_sum_fwd: C must be a multiple of the 16-byte vector");
  SumSrc s;
  for (int k = 0; k < 3; ++k) {
    s.p[k] = k < nsrc ? srcs[k] : nullptr;
    s.H[k] = k < nsrc ? hs[k] : 1;
    s.W[k] = k < nsrc ? ws[k] : 1;
    GDL_CHECK_ARG(k >= nsrc || (srcs[k] && hs[k] > 0 && ws[k] > 0 && (uintptr_t)srcs[k] % 16 == 0), "gdl_bilinear_sum_fwd: bad source %d", k);
  }
  GDL_CHECK_ARG((uintptr_t)out % 16 == 0, "gdl_bilinear_sum_fwd: out must be 16-byte aligned");
  const int vec = dtype == GDL_BF16 ? 8 : 4;
  GDL_CHECK_ARG((int64_t)B * Ho <= 65535, "gdl_bilinear_sum_fwd: B * Ho must fit one grid dimension");
  const dim3 grid((unsigned)((Wo * (C / vec) + 255) / 256), (unsigned)(B * Ho));
  if (dtype == GDL_BF16)
    hipLaunchKernelGGL((bilinear_sum_kernel<uint16_t, 8>), grid, dim3(256), 0, (hipStream_t)stream, s, nsrc, B, C, out, Ho, Wo);
  else
    hipLaunchKernelGGL((bilinear_sum_kernel<float, 4>), grid, dim3(256), 0, (hipStream_t)stream, s, nsrc, B, C, out, Ho, Wo);
  GDL_CHECK_LAUNCH("gdl_bilinear_sum_fwd");
  return GDL_OK;
}

extern "C" int gdl_bilinear_bwd(const void* dout, int dout_dtype, int B, int Ho, int Wo, int C, int64_t osB,
                                int64_t osH, int64_t osW, void* din, int din_dtype, int Hi, int Wi,
                                int64_t isB, int64_t isH, int64_t isW, int accumulate, gdl_stream_t stream) {
  GDL_CHECK_ARG(dout && din, "gdl_bilinear_bwd: null pointer");
  GDL_CHECK_ARG(C % 4 == 0 && isB % 4 == 0 && isH % 4 == 0 && isW % 4 == 0 && osB % 4 == 0 && osH % 4 == 0 &&
                    osW % 4 == 0, "gdl_bilinear_bwd: C and strides must be multiples of 4");
  if (dout_dtype == GDL_BF16 && din_dtype == GDL_BF16 && vec8_ok(dout, din, C, isB, isH, isW, osB, osH, osW)) {
    const int64_t total8 = (int64_t)B * Hi * Wi * (C / 8);
    const int nx = 2 * ((Wo + Wi - 1) / Wi) + 4;            // horizontal output window of one input pixel, upper bound
    const dim3 grid_rows((unsigned)((Wi * (C / 8) + 255) / 256), (unsigned)(B * Hi));
#define BWD_ROWS(NX) hipLaunchKernelGGL(bilinear_bwd8_rows_kernel<NX>, grid_rows, dim3(256), 0, (hipStream_t)stream, dout, Ho, \
                                        Wo, C, osB, osH, osW, din, Hi, Wi, isB, isH, isW, accumulate)
    const int fac = integer_factor(Hi, Wi, Ho, Wo);
    if ((fac == 2 || fac == 4) && (int64_t)B * ((Hi + 7) / 8) <= 65535 && !g_flat_resample) {
      const dim3 grid((unsigned)((Wi * (C / 8) + 255) / 256), (unsigned)(B * ((Hi + 7) / 8)));
      if (fac == 2) hipLaunchKernelGGL((bilinear_bwd8_walk_kernel<2, 8>), grid, dim3(256), 0, (hipStream_t)stream, dout, C, osB, osH, osW, din, Hi, Wi, isB, isH, isW, accumulate);
      else hipLaunchKernelGGL((bilinear_bwd8_walk_kernel<4, 8>), grid, dim3(256), 0, (hipStream_t)stream, dout, C, osB, osH, osW, din, Hi, Wi, isB, isH, isW, accumulate);
    } else if ((int64_t)B * Hi <= 65535 && nx <= 20 && g_flat_resample != 1) {
      if (nx <= 8) BWD_ROWS(8); else if (nx <= 12) BWD_ROWS(12); else BWD_ROWS(20);
    } else if (nx > 20 && (int64_t)B * Hi * Wi <= 65535 && !g_flat_resample) {
      hipLaunchKernelGGL(bilinear_bwd8_window_kernel, dim3((unsigned)((C / 8 + 31) / 32), (unsigned)(B * Hi * Wi)), dim3(256), 0,
                         (hipStream_t)stream, dout, Ho, Wo, C, osB, osH, osW, din, Hi, Wi, isB, isH, isW, accumulate);
    } else
#undef BWD_ROWS
    hipLaunchKernelGGL(bilinear_bwd8_kernel, dim3(resample_grid_for(total8)), dim3(256), 0, (hipStream_t)stream, dout, B, Ho, Wo,
                       C, osB, osH, osW, din, Hi, Wi, isB, isH, isW, accumulate);
    GDL_CHECK_LAUNCH("gdl_bilinear_bwd");
    return GDL_OK;
  }
  const int64_t total = (int64_t)B * Hi * Wi * (C / 4);
  DISPATCH2(bilinear_bwd_kernel, dout_dtype, din_dtype, dim3(resample_grid_for(total)), dim3(256), 0,
            (hipStream_t)stream, dout, B, Ho, Wo, C, osB, osH, osW, din, Hi, Wi, isB, isH, isW, accumulate);
  GDL_CHECK_LAUNCH("gdl_bilinear_bwd");
  return GDL_OK;
}

extern "C" int gdl_adaptive_avgpool_fwd(const void* in, int dtype, int B, int Hi, int Wi, int C, int64_t isB,
                                        int64_t isH, int64_t isW, void* out, int out_dtype, int So,
                                        gdl_stream_t stream) {
  GDL_CHECK_ARG(in && out && So > 0, "gdl_adaptive_avgpool_fwd: bad args");
  GDL_CHECK_ARG(C % 4 == 0 && isB % 4 == 0 && isH % 4 == 0 && isW % 4 == 0, "gdl_adaptive_avgpool_fwd: C/strides % 4");
  const int64_t total = (int64_t)B * So * So * (C / 4);
  if ((Hi / So) * (Wi / So) >= 32 && (int64_t)B * So * So <= 65535 && !g_flat_resample) {      // large bins: rows split over 8 lane groups
    const dim3 grid((unsigned)((C / 4 + 31) / 32), (unsigned)(B * So * So));
    DISPATCH2(avgpool_fwd_split_kernel, dtype, out_dtype, grid, dim3(256), 0, (hipStream_t)stream, in, Hi, Wi, C, isB, isH, isW, out, So);
    GDL_CHECK_LAUNCH("gdl_adaptive_avgpool_fwd");
    return GDL_OK;
  }
  DISPATCH2(avgpool_fwd_kernel, dtype, out_dtype, dim3(resample_grid_for(total)), dim3(256), 0, (hipStream_t)stream, in,
            B, Hi, Wi, C, isB, isH, isW, out, So);
  GDL_CHECK_LAUNCH("gdl_adaptive_avgpool_fwd");
  return GDL_OK;
}

extern "C" int gdl_adaptive_avgpool_bwd(const void* dout, int dtype, int B, int So, int C, void* din,
                                        int din_dtype, int Hi, int Wi, int64_t isB, int64_t isH, int64_t isW,
                                        int accumulate, gdl_stream_t stream) {
  GDL_CHECK_ARG(dout && din && So > 0, "gdl_adaptive_avgpool_bwd: bad args");
  GDL_CHECK_ARG(C % 4 == 0 && isB % 4 == 0 && isH % 4 == 0 && isW % 4 == 0, "gdl_adaptive_avgpool_bwd: C/strides % 4");
  const int64_t total = (int64_t)B * Hi * Wi * (C / 4);
  DISPATCH2(avgpool_bwd_kernel, dtype, din_dtype, dim3(resample_grid_for(total)), dim3(256), 0, (hipStream_t)stream,
            dout, B, So, C, din, Hi, Wi, isB, isH, isW, accumulate);
  GDL_CHECK_LAUNCH("gdl_adaptive_avgpool_bwd");
  return GDL_OK;
}
