// What the resampling units share (resample.hip, resize_conv_bwd.hip, resize_conv_fwd.hip): the 4- and 8-channel vector
// accessors every kernel loads and stores through, the source index of the bilinear resize (src_index2 of bilinear_index.h),
// and the LDS row types of the matrix-core gathers (the forward gather-sum and the one-pass backward gather).
#pragma once
#include "bilinear_index.h"

namespace {

// four channels at element offset `off`, as f32 in registers
template <typename T> struct V4;
template <> struct V4<float> {
  typedef float elem;
  static __device__ __forceinline__ void ld(const void* p, int64_t off, float (&o)[4]) {
    const float4 v = *(const float4*)((const float*)p + off);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
  static __device__ __forceinline__ void st(void* p, int64_t off, const float (&o)[4]) {
    *(float4*)((float*)p + off) = make_float4(o[0], o[1], o[2], o[3]);
  }
};
template <> struct V4<uint16_t> {
  typedef uint16_t elem;
  static __device__ __forceinline__ void ld(const void* p, int64_t off, float (&o)[4]) {
    const uint2 v = *(const uint2*)((const uint16_t*)p + off);
    o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
    o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
  }
  static __device__ __forceinline__ void st(void* p, int64_t off, const float (&o)[4]) {
    *(uint2*)((uint16_t*)p + off) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
  }
};

// 8 x bf16 = one 16-byte access: the bf16 -> bf16 resamples run 8 channels per thread (half the index math per byte)
struct V8 {
  typedef uint16_t elem;
  static __device__ __forceinline__ void ld(const void* p, int64_t off, float (&o)[8]) {
    const uint4 v = *(const uint4*)((const uint16_t*)p + off);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[2 * e] = __uint_as_float(w[e] << 16); o[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u); }
  }
  static __device__ __forceinline__ void st(void* p, int64_t off, const float (&o)[8]) {
    *(uint4*)((uint16_t*)p + off) = make_uint4(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]),
                                               pack_bf16x2(o[6], o[7]));
  }
};

// ---- the matrix-core gathers: rows of 64 bf16 channels (128 B) staged in LDS by DMA and read back through ds_read_b64_tr_b16
typedef __attribute__((ext_vector_type(4))) short tm_s16x4_t;
typedef __attribute__((ext_vector_type(8))) short tm_s16x8_t;
typedef __attribute__((address_space(3))) tm_s16x4_t* tm_lds_s16x4_ptr;
constexpr unsigned kTmOob = 0x80000000u;                   // buffer offset beyond every source: the DMA leaves zeros in the row
__device__ __forceinline__ int tm_swz(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }   // 16-byte chunk swizzle of LDS row `row`

}  // namespace
