// The classifier head: the 1x1 convolution to K <= 16 classes (wave per pixel, MFMA, wide MFMA), its backward wrt features and
// weights, and the final reduction of the weight gradient that norm.hip's fused BatchNorm + head backward shares (head_final.h).
#include <atomic>

#include "gdl_common.h"
#include "head_final.h"

namespace {

// 1x1 conv to K<=16 classes: one wave per pixel, 4 channels per lane per step.
template <typename T, int K>
__global__ __launch_bounds__(256) void head_1x1_kernel(const void* __restrict__ feat, int64_t P, int C, int64_t f_sP,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       const float* __restrict__ chan_scale, int64_t pix_per_img,
                                                       float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= P) return;
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.f;
  const float* cs = chan_scale ? chan_scale + (p / pix_per_img) * C : nullptr;
  for (int c = lane * 4; c < C; c += 256) {
    float v[4];
    if constexpr (sizeof(T) == 4) {
      const float4 t = *(const float4*)((const float*)feat + p * f_sP + c);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
      const uint2 t = *(const uint2*)((const uint16_t*)feat + p * f_sP + c);
      v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
      v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
    }
    if (cs) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] *= cs[c + j];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float4 ww = *(const float4*)(w + (int64_t)k * C + c);
      acc[k] += (v[0] * ww.x + v[1] * ww.y) + (v[2] * ww.z + v[3] * ww.w);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float s = wave_sum(acc[k]);
    if (lane == 0) out[p * K + k] = s + (bias ? bias[k] : 0.f);
  }
}

// The same head as a skinny MFMA GEMM (round 5): D[class][pixel] = W[class][c] . feat[pixel][c] with v_mfma_f32_16x16x32_bf16.
// The wave-per-pixel kernel above runs at 1.3 TB/s on the decoder output (340 MB, 267 us at batch 32): every pixel re-reads the
// K x C weights through the L1 (10 bytes of L1 traffic per byte of features), spends ~100 VALU instructions on five 64-lane
// butterflies, and a wave lives for one 8-byte load per lane.  Here a wave owns 16-pixel tiles (16 x C bf16, contiguous in HBM):
//   * NKS coalesced 16-byte loads per lane fetch the tile (the NEXT tile's are issued before this tile's MFMAs: 8 KB in flight per
//     wave), a wave-private LDS slot re-shapes it into B fragments (chunk index XOR row: conflict-free both ways);
//   * the f32 weights live in registers as bf16 hi + lo fragments (w = hi + lo to 2^-17: f32-grade logits), two MFMAs per 32 channels;
//   * lane (pixel j, group g) ends with classes 4g .. 4g+3 of its pixel: 4-float stores.
// Dense bf16 features with C = 32 NKS and no Dropout2d scale; everything else takes the kernel above.
// BN (decoder tail): feat is the PRE-BatchNorm convolution output and the head's features z = bf16(relu(bn(feat))) are formed on the
// way from the load registers into the LDS slot -- the f32 expression and the one bf16 rounding of bn_apply_kernel (norm.hip), so the
// fragments are bit for bit what the head reads from bn_apply's output, which is then never written.  A lane's 16-byte pieces are
// always the same eight channels (1024 % ROW == 0): 24 per-channel constants in registers.
template <int NKS, bool BN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BN ? 2 : 3, BN ? 2 : 3))) void head_1x1_mfma_kernel(const uint16_t* __restrict__ feat, int64_t P, const float* __restrict__ w,
                                                            const float* __restrict__ bias, int K, float* __restrict__ out,
                                                            const float* __restrict__ mean, const float* __restrict__ var,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu) {
  constexpr int C = NKS * 32, ROW = C * 2, TILE = 16 * ROW;
  extern __shared__ __attribute__((aligned(16))) unsigned char hsm[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned char* st = hsm + wv * TILE;
  const int j = lane & 15, g = lane >> 4;
  bf16x8_t wh[NKS], wl[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x0 = j < K ? w[(int64_t)j * C + 32 * ks + 8 * g + 2 * e] : 0.f;
      const float x1 = j < K ? w[(int64_t)j * C + 32 * ks + 8 * g + 2 * e + 1] : 0.f;
      hi[e] = pack_bf16x2(x0, x1);
      lo[e] = pack_bf16x2(x0 - __uint_as_float(hi[e] << 16), x1 - __uint_as_float(hi[e] & 0xffff0000u));
    }
    wh[ks] = __builtin_bit_cast(bf16x8_t, make_uint4(hi[0], hi[1], hi[2], hi[3]));
    wl[ks] = __builtin_bit_cast(bf16x8_t, make_uint4(lo[0], lo[1], lo[2], lo[3]));
  }
  float bv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bv[r] = (bias && 4 * g + r < K) ? bias[4 * g + r] : 0.f;
  const int64_t ntiles = (P + 15) / 16, stride = (int64_t)gridDim.x * 4;
  uint4 rg[NKS];
  float mu[BN ? 8 : 1], sc[BN ? 8 : 1], be[BN ? 8 : 1];
  if constexpr (BN) {
    const int c0 = 8 * (lane % (ROW / 16));
#pragma unroll
    for (int e = 0; e < 8; ++e) { mu[e] = mean[c0 + e]; sc[e] = rsqrtf(var[c0 + e] + eps) * gamma[c0 + e]; be[e] = beta[c0 + e]; }
  }
  auto bn_relu = [&](const uint4& r) {
    const uint32_t in[4] = {r.x, r.y, r.z, r.w};
    uint32_t o[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const float a = (__uint_as_float(in[h] << 16) - mu[2 * h]) * sc[2 * h] + be[2 * h];
      const float b = (__uint_as_float(in[h] & 0xffff0000u) - mu[2 * h + 1]) * sc[2 * h + 1] + be[2 * h + 1];
      o[h] = pack_bf16x2(relu ? fmaxf(a, 0.f) : a, relu ? fmaxf(b, 0.f) : b);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
  };
  auto gload = [&](int64_t tile) {
    const unsigned char* base = (const unsigned char*)feat + tile * TILE;
#pragma unroll
    for (int u = 0; u < NKS; ++u) {
      const int off = u * 1024 + lane * 16;
      rg[u] = tile * 16 + off / ROW < P ? *(const uint4*)(base + off) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  int64_t t = (int64_t)blockIdx.x * 4 + wv;
  if (t < ntiles) gload(t);
  for (; t < ntiles; t += stride) {
#pragma unroll
    for (int u = 0; u < NKS; ++u) {
      const int off = u * 1024 + lane * 16, row = off / ROW, c = (off % ROW) >> 4;
      if constexpr (BN) *(uint4*)(st + row * ROW + ((c ^ (row & 15)) << 4)) = bn_relu(rg[u]);
      else *(uint4*)(st + row * ROW + ((c ^ (row & 15)) << 4)) = rg[u];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (wave-private slot: the LDS queue is in order, no barrier needed)
    if (t + stride < ntiles) gload(t + stride);
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const bf16x8_t fb = __builtin_bit_cast(bf16x8_t, *(const uint4*)(st + j * ROW + (((4 * ks + g) ^ j) << 4)));
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks], fb, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[ks], fb, acc, 0, 0, 0);
    }
    const int64_t p = t * 16 + j;
    if (p < P) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * g + r < K) out[p * K + 4 * g + r] = acc[r] + bv[r];
    }
    asm volatile("" ::: "memory");                          // the next tile's LDS writes stay behind this tile's fragment reads
  }
}

// The same for C = 256 NW channels and / or a Dropout2d channel scale (SegFormer's 768-wide decoder, segformer_mlp.py:64-65,120-125; the
// DOFA heads in training when the map's pixel count is a multiple of 16).  The NW waves of a workgroup each take a 256-channel slice
// of the SAME 16-pixel tile (their 128 weight registers are that slice's hi / lo fragments), the partial 16 x 16 products meet in the
// LDS and wave 0 adds them in a fixed order.  A workgroup walks a CONTIGUOUS range of tiles, so the image index changes a handful of
// times: with a channel scale the fragments are those of w * scale[image] (the scale folded into the weights in f32 before the
// hi / lo split -- the features stay the bf16 values in memory), rebuilt when the image changes.  pix_per_img % 16 == 0 then (no tile
// straddles two images).
template <int NW, bool SCALE>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(SCALE ? 2 : 3, SCALE ? 2 : 3)))   // (SCALE: rebuilding the fragments
void head_1x1_mfma_wide_kernel(                                                 //  mid-loop spills 55 registers at three waves per SIMD)
const uint16_t* __restrict__ feat, int64_t P, const float* __restrict__ w, const float* __restrict__ bias,
                               const float* __restrict__ chan_scale, int64_t pix_per_img, int K, float* __restrict__ out) {
  constexpr int NKS = 8, C = 256 * NW, ROW = 512, TILE = 16 * ROW;
  extern __shared__ __attribute__((aligned(16))) unsigned char hsm[];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned char* st = hsm + wv * TILE;
  f32x4_t* red = (f32x4_t*)(hsm + NW * TILE);      // [2][NW][64]
  const int j = lane & 15, g = lane >> 4;
  bf16x8_t wh[NKS], wl[NKS];
  auto load_w = [&](const float* cs) {
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      uint32_t hi[4], lo[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = wv * 256 + 32 * ks + 8 * g + 2 * e;
        float x0 = j < K ? w[(int64_t)j * C + c] : 0.f, x1 = j < K ? w[(int64_t)j * C + c + 1] : 0.f;
        if (SCALE) { x0 *= cs[c]; x1 *= cs[c + 1]; }
        hi[e] = pack_bf16x2(x0, x1);
        lo[e] = pack_bf16x2(x0 - __uint_as_float(hi[e] << 16), x1 - __uint_as_float(hi[e] & 0xffff0000u));
      }
      wh[ks] = __builtin_bit_cast(bf16x8_t, make_uint4(hi[0], hi[1], hi[2], hi[3]));
      wl[ks] = __builtin_bit_cast(bf16x8_t, make_uint4(lo[0], lo[1], lo[2], lo[3]));
    }
  };
  float bv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bv[r] = (bias && 4 * g + r < K) ? bias[4 * g + r] : 0.f;
  const int64_t ntiles = (P + 15) / 16;
  const int64_t tpb = (ntiles + gridDim.x - 1) / gridDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * tpb, t1 = t0 + tpb < ntiles ? t0 + tpb : ntiles;
  uint4 rg[NKS];
  auto gload = [&](int64_t tile) {
#pragma unroll
    for (int u = 0; u < NKS; ++u) {
      const int64_t row = tile * 16 + 2 * u + (lane >> 5);
      rg[u] = row < P ? *(const uint4*)(feat + row * C + wv * 256 + (lane & 31) * 8) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  if (!SCALE) load_w(nullptr);
  int64_t img = -1;
  int par = 0;
  if (t0 < t1) gload(t0);
  for (int64_t t = t0; t < t1; ++t) {
    if (SCALE) {
      const int64_t b = (t * 16) / pix_per_img;
      if (b != img) { img = b; load_w(chan_scale + b * C); }
    }
#pragma unroll
    for (int u = 0; u < NKS; ++u) {
      const int row = 2 * u + (lane >> 5), c = lane & 31;
      *(uint4*)(st + row * ROW + ((c ^ (row & 15)) << 4)) = rg[u];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (t + 1 < t1) gload(t + 1);
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const bf16x8_t fb = __builtin_bit_cast(bf16x8_t, *(const uint4*)(st + j * ROW + (((4 * ks + g) ^ j) << 4)));
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[ks], fb, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[ks], fb, acc, 0, 0, 0);
    }
    if (NW > 1) {
      red[(par * NW + wv) * 64 + lane] = acc;
      __syncthreads();          // one barrier per tile: the two parities of `red` alternate, wave 0 is past its reads of a parity
                                // before anyone passes the NEXT barrier and writes that parity again
      if (wv == 0) {
#pragma unroll
        for (int q = 1; q < NW; ++q) {
          const f32x4_t o = red[(par * NW + q) * 64 + lane];
          acc[0] += o[0]; acc[1] += o[1]; acc[2] += o[2]; acc[3] += o[3];
        }
      }
      par ^= 1;
    }
    const int64_t p = t * 16 + j;
    if (wv == 0 && p < P) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * g + r < K) out[p * K + 4 * g + r] = acc[r] + bv[r];
    }
    asm volatile("" ::: "memory");
  }
}

// backward of the 1x1 head wrt features and weights
//  dfeat[p,c] = sum_k dlog[p,k] * w[k,c] (* chan_scale) ; dw[k,c] = sum_p dlog[p,k]*feat[p,c]*cs ; db[k] = sum_p dlog[p,k]
template <typename T, int K>
__global__ __launch_bounds__(256) void head_1x1_bwd_feat_kernel(const float* __restrict__ dlog, int64_t P, int C,
                                                                const float* __restrict__ w,
                                                                const float* __restrict__ chan_scale,
                                                                int64_t pix_per_img, void* dfeat, int64_t d_sP) {
  const int cv = C / 4;
  const int64_t total = P * cv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t p = i / cv;
    const int c = (int)(i - p * cv) * 4;
    float g[K];
#pragma unroll
    for (int k = 0; k < K; ++k) g[k] = dlog[p * K + k];
    float o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float4 ww = *(const float4*)(w + (int64_t)k * C + c);
      o[0] += g[k] * ww.x; o[1] += g[k] * ww.y; o[2] += g[k] * ww.z; o[3] += g[k] * ww.w;
    }
    if (chan_scale) {
      const float* cs = chan_scale + (p / pix_per_img) * C + c;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] *= cs[j];
    }
    if constexpr (sizeof(T) == 4) *(float4*)((float*)dfeat + p * d_sP + c) = make_float4(o[0], o[1], o[2], o[3]);
    else *(uint2*)((uint16_t*)dfeat + p * d_sP + c) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
  }
}

// The same for dense bf16 gradients with the weights in registers (round 5): a lane owns EIGHT fixed channels (one 16-byte store) and
// walks pixels; the kernel above re-reads its K float4 weight vectors from the L1 for every 8 bytes it stores (164 us for 340 MB).
// Per-element arithmetic: the same products added in the same order, as explicit fused multiply-adds.  256 % (C / 8) == 0, no
// Dropout2d scale.
template <int K>
__global__ __launch_bounds__(256) void head_1x1_bwd_feat8_kernel(const float* __restrict__ dlog, int64_t P, int C,
                                                                 const float* __restrict__ w, uint16_t* __restrict__ dfeat) {
  const int cv = C >> 3, q = threadIdx.x % cv, ro = threadIdx.x / cv, rpb = 256 / cv;
  float wr[K][8];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float4 a = *(const float4*)(w + (int64_t)k * C + q * 8), b = *(const float4*)(w + (int64_t)k * C + q * 8 + 4);
    wr[k][0] = a.x; wr[k][1] = a.y; wr[k][2] = a.z; wr[k][3] = a.w; wr[k][4] = b.x; wr[k][5] = b.y; wr[k][6] = b.z; wr[k][7] = b.w;
  }
  const int64_t step = (int64_t)gridDim.x * rpb;
  auto one = [&](int64_t p, const float (&gk)[K]) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fmaf(gk[k], wr[k][e], o[e]);
    }
    *(uint4*)(dfeat + p * C + q * 8) = make_uint4(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7]));
  };
  int64_t p = (int64_t)blockIdx.x * rpb + ro;
  for (; p + 3 * step < P; p += 4 * step) {       // four pixels' gradients requested before the first is used
    float gk[4][K];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int k = 0; k < K; ++k) gk[u][k] = dlog[(p + u * step) * K + k];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) one(p + u * step, gk[u]);
  }
  for (; p < P; p += step) {
    float gk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) gk[k] = dlog[p * K + k];
    one(p, gk);
  }
}

// dw partials: grid (C/256, nsplit); each lane 4 channels; ws[split][K][C]; db via extra row K
template <typename T, int K>
__global__ __launch_bounds__(256) void head_1x1_bwd_w_partial(const void* __restrict__ feat, const float* __restrict__ dlog,
                                                              int64_t P, int C, int64_t f_sP,
                                                              const float* __restrict__ chan_scale,
                                                              int64_t pix_per_img, float* __restrict__ ws) {
  __shared__ float red[4][K][256];
  __shared__ float redb[4][K];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = blockIdx.x * 256 + lane * 4;
  const int nsplit = gridDim.y;
  const int64_t per = (P + nsplit - 1) / nsplit;
  const int64_t p0 = per * blockIdx.y, p1 = p0 + per < P ? p0 + per : P;
  float acc[K][4];
  float accb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { accb[k] = 0.f; acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.f; }
  auto load = [&](int64_t p, float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (c < C) {
      if constexpr (sizeof(T) == 4) {
        const float4 t = *(const float4*)((const float*)feat + p * f_sP + c);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else {
        const uint2 t = *(const uint2*)((const uint16_t*)feat + p * f_sP + c);
        v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
        v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
      }
      if (chan_scale) {
        const float* cs = chan_scale + (p / pix_per_img) * C + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] *= cs[j];
      }
    }
  };
  auto add = [&](int64_t p, const float (&v)[4]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float g = dlog[p * K + k];
      accb[k] += g;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[k][j] += g * v[j];
    }
  };
  int64_t p = p0 + wv;
  for (; p + 12 < p1; p += 16) {      // four pixel rows in flight per wave (one at a time ran at 2 TB/s), same summation order
    // (round 5: eight rows in flight need 134 registers -- three waves per SIMD -- and run 1.6 x SLOWER; a forward kernel that
    //  walks 16-pixel runs per wave with four rows in flight loses the same way: 243 us against 133 -- profiles/r05n_*)
    float v[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) load(p + 4 * u, v[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) add(p + 4 * u, v[u]);
  }
  for (; p < p1; p += 4) {
    float v[4];
    load(p, v);
    add(p, v);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < 4; ++j) red[wv][k][lane * 4 + j] = acc[k][j];
    if (lane == 0) redb[wv][k] = accb[k];
  }
  __syncthreads();
  const int t = threadIdx.x, cc = blockIdx.x * 256 + t;
  float* wsb = ws + (int64_t)blockIdx.y * (K + 1) * C;
  if (cc < C) {
#pragma unroll
    for (int k = 0; k < K; ++k) wsb[(int64_t)k * C + cc] = (red[0][k][t] + red[1][k][t]) + (red[2][k][t] + red[3][k][t]);
  }
  if (blockIdx.x == 0 && t < K) wsb[(int64_t)K * C + t] = (redb[0][t] + redb[1][t]) + (redb[2][t] + redb[3][t]);
}

// dw partials for dense bf16 features (round 5): the shape of bn_bwd_partial8 -- a workgroup owns whole pixel rows, a lane EIGHT fixed
// channels (16-byte loads), four rows requested before the first is used (4 KB in flight per wave; the kernel above keeps 2 KB and
// pays one L2 round trip for the gradients after every batch of feature loads: 1.5-1.9 TB/s).  256 % (C / 8) == 0, K <= 8.
template <int K>
__global__ __launch_bounds__(256) void head_1x1_bwd_w_partial8(const uint16_t* __restrict__ feat, const float* __restrict__ dlog,
                                                               int64_t P, int C, float* __restrict__ ws) {
  __shared__ float red[256][9];             // [thread][channel | bias term] (+1: bank spread)
  const int G = C >> 3, R = 256 / G;        // lanes per pixel, pixel rows per block step
  const int t = threadIdx.x, g = t % G, prow = t / G;
  const int nsplit = gridDim.x;
  const int64_t per = (P + nsplit - 1) / nsplit;
  const int64_t p0 = per * blockIdx.x, p1 = p0 + per < P ? p0 + per : P;
  float acc[K][8], accb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    accb[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
  }
  auto add = [&](const uint4& xv, const float (&gk)[K]) {
    float v[8];
    v[0] = __uint_as_float(xv.x << 16); v[1] = __uint_as_float(xv.x & 0xffff0000u);
    v[2] = __uint_as_float(xv.y << 16); v[3] = __uint_as_float(xv.y & 0xffff0000u);
    v[4] = __uint_as_float(xv.z << 16); v[5] = __uint_as_float(xv.z & 0xffff0000u);
    v[6] = __uint_as_float(xv.w << 16); v[7] = __uint_as_float(xv.w & 0xffff0000u);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      accb[k] += gk[k];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(gk[k], v[j], acc[k][j]);
    }
  };
  int64_t p = p0 + prow;
  for (; p + 3 * R < p1; p += 4 * R) {
    uint4 xv[4];
    float gk[4][K];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      xv[u] = *(const uint4*)(feat + (p + (int64_t)u * R) * C + 8 * g);
#pragma unroll
      for (int k = 0; k < K; ++k) gk[u][k] = dlog[(p + (int64_t)u * R) * K + k];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) add(xv[u], gk[u]);
  }
  for (; p < p1; p += R) {
    float gk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) gk[k] = dlog[p * K + k];
    add(*(const uint4*)(feat + p * C + 8 * g), gk);
  }
  float* wsb = ws + (int64_t)blockIdx.x * (K + 1) * C;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[t][j] = acc[k][j];
    red[t][8] = accb[k];
    __syncthreads();
    for (int c = t; c < C; c += 256) {
      float ss = 0.f;
      for (int r = 0; r < R; ++r) ss += red[r * G + (c >> 3)][c & 7];
      wsb[(int64_t)k * C + c] = ss;
    }
    if (t == 0) {
      float sb = 0.f;
      for (int r = 0; r < R; ++r) sb += red[r * G][8];
      wsb[(int64_t)K * C + k] = sb;
    }
    __syncthreads();
  }
}

// General forms of the two kernels above: TPB = 256 or 192 threads (C / 8 lanes per pixel must divide it: 96 lanes for SegFormer's 768
// channels) and an optional Dropout2d channel scale, held per lane for the image it is working in (a workgroup walks a contiguous
// pixel range: the eight scale values are re-read a handful of times).  Arithmetic as in the 4-channel kernels: the scale multiplies
// the finished feature-gradient sum / the feature value before it enters the weight-gradient sum.
template <int K, int TPB, bool SCALE>
__global__ __launch_bounds__(TPB) void head_1x1_bwd_feat8g_kernel(const float* __restrict__ dlog, int64_t P, int C, const float* __restrict__ w,
                                                                  const float* __restrict__ chan_scale, int64_t pix_per_img,
                                                                  uint16_t* __restrict__ dfeat) {
  const int G = C >> 3, q = threadIdx.x % G, ro = threadIdx.x / G, R = TPB / G;
  float wr[K][8];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float4 a = *(const float4*)(w + (int64_t)k * C + q * 8), b = *(const float4*)(w + (int64_t)k * C + q * 8 + 4);
    wr[k][0] = a.x; wr[k][1] = a.y; wr[k][2] = a.z; wr[k][3] = a.w; wr[k][4] = b.x; wr[k][5] = b.y; wr[k][6] = b.z; wr[k][7] = b.w;
  }
  const int64_t per = (P + gridDim.x - 1) / gridDim.x;
  const int64_t p0 = per * blockIdx.x, p1 = p0 + per < P ? p0 + per : P;
  float csr[8];
  int64_t bc = -1;
  auto one = [&](int64_t p, const float (&gk)[K]) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fmaf(gk[k], wr[k][e], o[e]);
    }
    if (SCALE) {
      const int64_t b = p / pix_per_img;
      if (b != bc) {
        bc = b;
        const float4 a = *(const float4*)(chan_scale + b * C + q * 8), c4 = *(const float4*)(chan_scale + b * C + q * 8 + 4);
        csr[0] = a.x; csr[1] = a.y; csr[2] = a.z; csr[3] = a.w; csr[4] = c4.x; csr[5] = c4.y; csr[6] = c4.z; csr[7] = c4.w;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] *= csr[e];
    }
    *(uint4*)(dfeat + p * C + q * 8) = make_uint4(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7]));
  };
  if (ro >= R) return;
  int64_t p = p0 + ro;
  for (; p + 3 * R < p1; p += 4 * R) {
    float gk[4][K];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int k = 0; k < K; ++k) gk[u][k] = dlog[(p + (int64_t)u * R) * K + k];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) one(p + (int64_t)u * R, gk[u]);
  }
  for (; p < p1; p += R) {
    float gk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) gk[k] = dlog[p * K + k];
    one(p, gk);
  }
}

template <int K, int TPB, bool SCALE>
__global__ __launch_bounds__(TPB) void head_1x1_bwd_w_partial8g(const uint16_t* __restrict__ feat, const float* __restrict__ dlog, int64_t P,
                                                                int C, const float* __restrict__ chan_scale, int64_t pix_per_img,
                                                                float* __restrict__ ws) {
  __shared__ float red[TPB][9];
  const int G = C >> 3, R = TPB / G;
  const int t = threadIdx.x, g = t % G, prow = t / G;
  const int nsplit = gridDim.x;
  const int64_t per = (P + nsplit - 1) / nsplit;
  const int64_t p0 = per * blockIdx.x, p1 = p0 + per < P ? p0 + per : P;
  float acc[K][8], accb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    accb[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
  }
  float csr[8];
  int64_t bc = -1;
  auto add = [&](int64_t p, const uint4& xv, const float (&gk)[K]) {
    float v[8];
    v[0] = __uint_as_float(xv.x << 16); v[1] = __uint_as_float(xv.x & 0xffff0000u);
    v[2] = __uint_as_float(xv.y << 16); v[3] = __uint_as_float(xv.y & 0xffff0000u);
    v[4] = __uint_as_float(xv.z << 16); v[5] = __uint_as_float(xv.z & 0xffff0000u);
    v[6] = __uint_as_float(xv.w << 16); v[7] = __uint_as_float(xv.w & 0xffff0000u);
    if (SCALE) {
      const int64_t b = p / pix_per_img;
      if (b != bc) {
        bc = b;
        const float4 a = *(const float4*)(chan_scale + b * C + g * 8), c4 = *(const float4*)(chan_scale + b * C + g * 8 + 4);
        csr[0] = a.x; csr[1] = a.y; csr[2] = a.z; csr[3] = a.w; csr[4] = c4.x; csr[5] = c4.y; csr[6] = c4.z; csr[7] = c4.w;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= csr[j];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      accb[k] += gk[k];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(gk[k], v[j], acc[k][j]);
    }
  };
  if (prow < R) {
    int64_t p = p0 + prow;
    for (; p + 3 * R < p1; p += 4 * R) {
      uint4 xv[4];
      float gk[4][K];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        xv[u] = *(const uint4*)(feat + (p + (int64_t)u * R) * C + 8 * g);
#pragma unroll
        for (int k = 0; k < K; ++k) gk[u][k] = dlog[(p + (int64_t)u * R) * K + k];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) add(p + (int64_t)u * R, xv[u], gk[u]);
    }
    for (; p < p1; p += R) {
      float gk[K];
#pragma unroll
      for (int k = 0; k < K; ++k) gk[k] = dlog[p * K + k];
      add(p, *(const uint4*)(feat + p * C + 8 * g), gk);
    }
  }
  float* wsb = ws + (int64_t)blockIdx.x * (K + 1) * C;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[t][j] = acc[k][j];
    red[t][8] = accb[k];
    __syncthreads();
    for (int c = t; c < C; c += TPB) {
      float ss = 0.f;
      for (int r = 0; r < R; ++r) ss += red[r * G + (c >> 3)][c & 7];
      wsb[(int64_t)k * C + c] = ss;
    }
    if (t == 0) {
      float sb = 0.f;
      for (int r = 0; r < R; ++r) sb += red[r * G][8];
      wsb[(int64_t)K * C + k] = sb;
    }
    __syncthreads();
  }
}

template <int K>
__global__ __launch_bounds__(1024) void head_1x1_bwd_w_final(const float* __restrict__ ws, int nsplit, int C,
                                                             float* __restrict__ dw, float* __restrict__ db) {
  // outputs 0..K*C-1 = dw, K*C..K*C+K-1 = db; block = 8 outputs x 128 split groups (round 5: up to 2048 partial rows)
  __shared__ double part[128][8];
  const int cl = threadIdx.x & 7, grp = threadIdx.x >> 3;
  const int i = blockIdx.x * 8 + cl;
  const int total = K * C + (db ? K : 0);
  double s = 0;
  if (i < total) {
    const int64_t off = i < K * C ? i : (int64_t)K * C + (i - K * C);
    s = ordered_sum8<double>(grp, nsplit, 128, [&](int sp) { return ws[(int64_t)sp * (K + 1) * C + off]; });
  }
  part[grp][cl] = s;
  __syncthreads();
  if (grp < 8) {          // 128 -> 8 -> 1, fixed order
    s = 0;
#pragma unroll
    for (int g = 0; g < 16; ++g) s += part[grp * 16 + g][cl];
  }
  __syncthreads();
  if (grp < 8) part[grp][cl] = s;
  __syncthreads();
  if (grp != 0 || i >= total) return;
  s = 0;
#pragma unroll
  for (int g = 0; g < 8; ++g) s += part[g][cl];
  if (i < K * C) dw[i] = (float)s;
  else db[i - K * C] = (float)s;
}

}  // namespace

// A/B hook: 0 = the round-4 head kernels (wave per pixel forward, L1-resident weights in the feature gradient) for every shape
static std::atomic<int> g_head_mfma{1};
extern "C" void gdl_debug_set_head_mfma(int on) { g_head_mfma = on; }

extern "C" int gdl_head_1x1(const void* feat, int dtype, int64_t P, int C, int64_t f_sP, const float* w,
                            const float* bias, const float* chan_scale, int64_t pix_per_img, float* out, int K,
                            gdl_stream_t stream) {
  GDL_CHECK_ARG(feat && w && out && C % 4 == 0 && f_sP % 4 == 0 && pix_per_img > 0, "gdl_head_1x1: bad args");
  hipStream_t s = (hipStream_t)stream;
  if (g_head_mfma.load(std::memory_order_relaxed) && dtype == GDL_BF16 && !chan_scale && f_sP == C && (C == 128 || C == 256) && K >= 1 &&
      K <= 16 && P >= 1024 && (uintptr_t)feat % 16 == 0) {
    const int64_t ntiles = (P + 15) / 16;
    const int cap = 3 * gdl_num_cus();     // all workgroups resident at once (156 registers: three waves per SIMD), each wave walks its share
    const unsigned blocks = (unsigned)((ntiles + 3) / 4 < cap ? (ntiles + 3) / 4 : cap);
    const float* none = nullptr;
    if (C == 256) hipLaunchKernelGGL((head_1x1_mfma_kernel<8, false>), dim3(blocks), dim3(256), 4 * 16 * 512, s, (const uint16_t*)feat, P, w, bias, K, out, none, none, none, none, 0.f, 0);
    else hipLaunchKernelGGL((head_1x1_mfma_kernel<4, false>), dim3(blocks), dim3(256), 4 * 16 * 256, s, (const uint16_t*)feat, P, w, bias, K, out, none, none, none, none, 0.f, 0);
    GDL_CHECK_LAUNCH("gdl_head_1x1(mfma)");
    return GDL_OK;
  }
  if (g_head_mfma.load(std::memory_order_relaxed) && dtype == GDL_BF16 && f_sP == C && C % 256 == 0 && C <= 1024 && K >= 1 && K <= 16 &&
      P >= 1024 && (uintptr_t)feat % 16 == 0 && (!chan_scale || pix_per_img % 16 == 0)) {
    // 256 NW channels and / or a Dropout2d scale: NW waves per tile, contiguous tile ranges
    const int NW = C / 256;
    const int64_t ntiles = (P + 15) / 16;
    const int64_t cap = (int64_t)((chan_scale ? 8 : 12) / NW) * gdl_num_cus();      // every workgroup resident: 2 / 3 waves per SIMD
    const unsigned blocks = (unsigned)(ntiles < cap ? ntiles : cap);
    const size_t lds = (size_t)NW * (16 * 512 + 2 * 64 * 16);
    const uint16_t* f = (const uint16_t*)feat;
#define GDL_HEAD_WIDE(NWV, SC) hipLaunchKernelGGL((head_1x1_mfma_wide_kernel<NWV, SC>), dim3(blocks), dim3(64 * NWV), lds, s, f, P, w, bias, chan_scale, pix_per_img, K, out)
    switch (NW * 2 + (chan_scale ? 1 : 0)) {
      case 2: GDL_HEAD_WIDE(1, false); break;
      case 3: GDL_HEAD_WIDE(1, true); break;
      case 4: GDL_HEAD_WIDE(2, false); break;
      case 5: GDL_HEAD_WIDE(2, true); break;
      case 6: GDL_HEAD_WIDE(3, false); break;
      case 7: GDL_HEAD_WIDE(3, true); break;
      case 8: GDL_HEAD_WIDE(4, false); break;
      default: GDL_HEAD_WIDE(4, true); break;
    }
#undef GDL_HEAD_WIDE
    GDL_CHECK_LAUNCH("gdl_head_1x1(mfma, wide)");
    return GDL_OK;
  }
  const unsigned grid = (unsigned)((P + 3) / 4);
  K_SWITCH(K, if (dtype == GDL_BF16) hipLaunchKernelGGL((head_1x1_kernel<uint16_t, KK>), dim3(grid), dim3(256), 0, s, feat, P, C, f_sP, w, bias, chan_scale, pix_per_img, out);
              else hipLaunchKernelGGL((head_1x1_kernel<float, KK>), dim3(grid), dim3(256), 0, s, feat, P, C, f_sP, w, bias, chan_scale, pix_per_img, out));
  GDL_CHECK_LAUNCH("gdl_head_1x1");
  return GDL_OK;
}

// The 256-channel head over relu?(bn(x)) without the normalised map (decoder tail in training): x is the saved convolution output,
// the features are formed inside head_1x1_mfma_kernel<8, true>.  Dense bf16, C == 256, K <= 8, P >= 4096 (gdl_head_1x1_bn_ok: the
// range of the backward that goes with it, gdl_bn_head_bwd_ok); every other shape is an error -- the caller runs gdl_bn_apply +
// gdl_head_1x1 there.  gdl_debug_set_head_mfma does not reach this form (there is no wave-per-pixel kernel with BatchNorm on load).
extern "C" int gdl_head_1x1_bn_ok(int dtype, int64_t P, int C, int K) {
  return dtype == GDL_BF16 && C == 256 && K >= 1 && K <= 8 && P >= 4096;
}

extern "C" int gdl_head_1x1_bn(const void* x, int dtype, int64_t P, int C, const float* mean, const float* var, const float* gamma,
                               const float* beta, float eps, int relu, const float* w, const float* bias, float* out, int K,
                               gdl_stream_t stream) {
  GDL_CHECK_ARG(x && mean && var && gamma && beta && w && out, "gdl_head_1x1_bn: null pointer");
  GDL_CHECK_ARG(gdl_head_1x1_bn_ok(dtype, P, C, K) && (uintptr_t)x % 16 == 0,
                "gdl_head_1x1_bn: needs dense 16-byte aligned bf16 features with C == 256, K <= 8, P >= 4096");
  const int64_t ntiles = (P + 15) / 16;
  const int cap = 2 * gdl_num_cus();       // all workgroups resident at once (two waves per SIMD), each wave walks its share
  const unsigned blocks = (unsigned)((ntiles + 3) / 4 < cap ? (ntiles + 3) / 4 : cap);
  hipLaunchKernelGGL((head_1x1_mfma_kernel<8, true>), dim3(blocks), dim3(256), 4 * 16 * 512, (hipStream_t)stream, (const uint16_t*)x, P, w,
                     bias, K, out, mean, var, gamma, beta, eps, relu);
  GDL_CHECK_LAUNCH("gdl_head_1x1_bn");
  return GDL_OK;
}

// final reduction of head weight-gradient partial rows ws[nsplit][K + 1][C] written by another translation unit's kernel
// (gdl_bn_head_bwd_reduce, norm.hip): the last launch of gdl_head_1x1_bwd
int head_bwd_w_final_launch(const float* ws, int nsplit, int C, int K, float* dw, float* db, hipStream_t s) {
  K_SWITCH(K, hipLaunchKernelGGL((head_1x1_bwd_w_final<KK>), dim3((KK * C + KK + 7) / 8), dim3(1024), 0, s, ws, nsplit, C, dw, db));
  return GDL_OK;
}

// partial rows of the weight gradient: one workgroup each.  Round 5: up to 2048 (eight workgroups per CU) -- with 512 the main head's
// 340 MB were read by two workgroups per CU, 16 KB in flight per CU: 1.5 TB/s
static int head_bwd_nsplit(int64_t P) {
  int64_t ns = P / 256; if (ns < 1) ns = 1; if (ns > 2048) ns = 2048;
  return (int)ns;
}

extern "C" int64_t gdl_head_1x1_bwd_workspace(int64_t P, int C, int K) {
  return (int64_t)head_bwd_nsplit(P) * (K + 1) * (int64_t)C * sizeof(float);
}

extern "C" int gdl_head_1x1_bwd(const void* feat, int dtype, const float* dlog, int64_t P, int C, int64_t f_sP,
                                const float* w, const float* chan_scale, int64_t pix_per_img, void* dfeat,
                                int64_t d_sP, float* dw, float* db, int K, float* ws, int64_t ws_bytes,
                                gdl_stream_t stream) {
  GDL_CHECK_ARG(feat && dlog && w && dw && ws && C % 4 == 0 && f_sP % 4 == 0, "gdl_head_1x1_bwd: bad args");
  GDL_CHECK_ARG(ws_bytes >= gdl_head_1x1_bwd_workspace(P, C, K), "gdl_head_1x1_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int nsplit = head_bwd_nsplit(P);
  dim3 gridw((C + 255) / 256, nsplit);
  const int64_t total = P * (C / 4);
  const bool feat8 = g_head_mfma.load(std::memory_order_relaxed) && dtype == GDL_BF16 && dfeat && !chan_scale && d_sP == C && C % 8 == 0 &&
                     C / 8 <= 256 && 256 % (C / 8) == 0 && K <= 8 && (uintptr_t)dfeat % 16 == 0 && P >= 1024 &&
                     (uintptr_t)w % 16 == 0;      // (the kernel reads the weights with float4 loads: a view at an odd offset takes the general path)
  // general wide forms (a Dropout2d scale, or C / 8 lanes per pixel that only divide 192 threads: SegFormer's 768 channels)
  const int G8 = C % 8 == 0 ? C / 8 : 0;
  const int tpb = G8 == 0 ? 0 : (G8 <= 256 && 256 % G8 == 0) ? 256 : (G8 <= 192 && 192 % G8 == 0) ? 192 : 0;
  const bool gen_ok = g_head_mfma.load(std::memory_order_relaxed) && dtype == GDL_BF16 && tpb != 0 && K <= 8 && P >= 1024 &&
                      (uintptr_t)chan_scale % 16 == 0 && (uintptr_t)w % 16 == 0 && (chan_scale || tpb == 192);
  const bool feat8g = gen_ok && dfeat && !feat8 && d_sP == C && (uintptr_t)dfeat % 16 == 0;
  const bool w8g = gen_ok && f_sP == C && (uintptr_t)feat % 16 == 0;
  K_SWITCH(K,
    if (dtype == GDL_BF16) {
      if constexpr (KK <= 8) {
        if (feat8g) {
          const dim3 gg(4 * gdl_num_cus());
          if (tpb == 256) hipLaunchKernelGGL((head_1x1_bwd_feat8g_kernel<KK, 256, true>), gg, dim3(256), 0, s, dlog, P, C, w, chan_scale, pix_per_img, (uint16_t*)dfeat);
          else if (chan_scale) hipLaunchKernelGGL((head_1x1_bwd_feat8g_kernel<KK, 192, true>), gg, dim3(192), 0, s, dlog, P, C, w, chan_scale, pix_per_img, (uint16_t*)dfeat);
          else hipLaunchKernelGGL((head_1x1_bwd_feat8g_kernel<KK, 192, false>), gg, dim3(192), 0, s, dlog, P, C, w, chan_scale, pix_per_img, (uint16_t*)dfeat);
        }
        if (w8g) {
          if (tpb == 256) hipLaunchKernelGGL((head_1x1_bwd_w_partial8g<KK, 256, true>), dim3(nsplit), dim3(256), 0, s, (const uint16_t*)feat, dlog, P, C, chan_scale, pix_per_img, ws);
          else if (chan_scale) hipLaunchKernelGGL((head_1x1_bwd_w_partial8g<KK, 192, true>), dim3(nsplit), dim3(192), 0, s, (const uint16_t*)feat, dlog, P, C, chan_scale, pix_per_img, ws);
          else hipLaunchKernelGGL((head_1x1_bwd_w_partial8g<KK, 192, false>), dim3(nsplit), dim3(192), 0, s, (const uint16_t*)feat, dlog, P, C, chan_scale, pix_per_img, ws);
        }
        if (feat8) hipLaunchKernelGGL((head_1x1_bwd_feat8_kernel<KK>), dim3(4 * gdl_num_cus()), dim3(256), 0, s, dlog, P, C, w, (uint16_t*)dfeat);   // (all resident at once: 74 registers allow six waves per SIMD, 8 per CU left a third of the grid for a second round)
      }
      if (dfeat && !feat8 && !feat8g) hipLaunchKernelGGL((head_1x1_bwd_feat_kernel<uint16_t, KK>), dim3(grid_for(total)), dim3(256), 0, s, dlog, P, C, w, chan_scale, pix_per_img, dfeat, d_sP);
      bool w8 = false;
      if constexpr (KK <= 8) {
        w8 = g_head_mfma.load(std::memory_order_relaxed) && !chan_scale && f_sP == C && C % 8 == 0 && C / 8 <= 256 && 256 % (C / 8) == 0 &&
             (uintptr_t)feat % 16 == 0 && P >= 1024;
        if (w8) hipLaunchKernelGGL((head_1x1_bwd_w_partial8<KK>), dim3(nsplit), dim3(256), 0, s, (const uint16_t*)feat, dlog, P, C, ws);
      }
      if (!w8 && !w8g) hipLaunchKernelGGL((head_1x1_bwd_w_partial<uint16_t, KK>), gridw, dim3(256), 0, s, feat, dlog, P, C, f_sP, chan_scale, pix_per_img, ws);
    } else {
      if (dfeat) hipLaunchKernelGGL((head_1x1_bwd_feat_kernel<float, KK>), dim3(grid_for(total)), dim3(256), 0, s, dlog, P, C, w, chan_scale, pix_per_img, dfeat, d_sP);
      hipLaunchKernelGGL((head_1x1_bwd_w_partial<float, KK>), gridw, dim3(256), 0, s, feat, dlog, P, C, f_sP, chan_scale, pix_per_img, ws);
    }
    hipLaunchKernelGGL((head_1x1_bwd_w_final<KK>), dim3((KK * C + KK + 7) / 8), dim3(1024), 0, s, ws, nsplit, C, dw, db));
  GDL_CHECK_LAUNCH("gdl_head_1x1_bwd");
  return GDL_OK;
}
