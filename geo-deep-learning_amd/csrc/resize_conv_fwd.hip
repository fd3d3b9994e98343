// Forward gather-sum ("tapsum") of the resized 3x3 convolutions (their backward gather: resize_conv_bwd.hip).  In order: the kernels
// (pixel kernel, matrix-core versions 1 and 2, the rolling-window kernels roll and roll3, the any-ratio kernel), the planner (TapPlan,
// tapsum_plan: every choice between them), the launcher (tapsum_launch) and the gdl_resize_conv3x3_fwd_sum* entry points.
#include "gdl_common.h"
#include "resample_vec.h"
#include <atomic>
#include <type_traits>

namespace {

// FORWARD of  y = conv3x3(pad 1)(bilinear_resize(x))  at LOW resolution (the transpose of the gather of resize_conv_bwd.hip).
//   y = sum_t W_t (S_t U x) = sum_t S_t U (W_t x)        (U, S_t act on pixels, W_t on channels: they commute)
// so the nine tap products z_t = W_t x are ONE 1x1 convolution over the low-resolution pixels with 9 N output channels
// (1 / factor^2 of the MACs of the convolution on the upsampled map), and what is left is this kernel:
//   y[b, oy, ox, n] = sum_{r,s} [0 <= oy+r-1 < Ho][0 <= ox+s-1 < Wo]  bilinear(z_(r,s))[oy + r - 1, ox + s - 1]
// z dense [B, Hi, Wi, 9 N], tap block t = 3 r + s.  Up to three sources of different (integer) factors are summed into one
// output (UperNet's fpn_bottleneck over its upsampled levels); the upsampled maps and the concat buffer never exist.
// A thread owns RUN consecutive output pixels of one row x VEC channels.  For a source of factor F the run is RUN / F cells
// (one cell = the F outputs that share a low-resolution column triple): per cell the nine taps are first combined
// vertically into h[s][column] (54 vector loads: 3 filter rows x 2 source rows x 3 taps x 3 columns), then every output of
// the cell takes 9 multiply-adds from h -- 54/F + 9 multiply-adds per output element instead of 36 for pixel-by-pixel
// sampling.  f32 accumulation in a fixed order, no atomics.
struct TapSrc { const void* p[3]; int H[3], W[3], F[3]; };

template <typename V, int VEC, int RUN, int F>
__device__ __forceinline__ void tapsum_source(float (&acc)[RUN][VEC], const void* __restrict__ z, int Hi, int Wi, int N, int b,
                                              int oy, int Ho, int ox0, int Wo, int c) {
  constexpr int CELLS = RUN / F;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  const int pix = 9 * N;                                           // elements per low-resolution pixel
  const char* zb = (const char*)z + (int64_t)b * Hi * Wi * pix * (int64_t)sizeof(typename V::elem);   // this image (uniform)
#pragma unroll 1
  for (int cell = 0; cell < CELLS; ++cell) {
    const int ix = ox0 / F + cell;
    float wx[F + 2][3];                            // wx[pos][k]: weight of source column ix - 1 + k for position ix*F - 1 + pos
#pragma unroll
    for (int pos = 0; pos < F + 2; ++pos) {
      const int px = ix * F - 1 + pos;
      int x0 = -9, x1 = -9; float lx = 0.f;
      const bool in = px >= 0 && px < Wo;
      if (in) src_index2(rx, px, Wi, x0, x1, lx);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int col = ix - 1 + k;
        wx[pos][k] = in ? ((x0 == col ? 1.f - lx : 0.f) + (x1 == col ? lx : 0.f)) : 0.f;
      }
    }
    int coff[3];                                   // out-of-image columns are clamped: their weights are zero
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      int col = ix - 1 + k;
      col = col < 0 ? 0 : (col > Wi - 1 ? Wi - 1 : col);
      coff[k] = col * pix + c;
    }
    float h[3][3][VEC];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int e = 0; e < VEC; ++e) h[s][k][e] = 0.f;
#pragma unroll 1
    for (int r = 0; r < 3; ++r) {                  // filter row r reads output row oy + r - 1 of the (virtual) upsampled map
      const int py = oy + r - 1;
      if (py < 0 || py >= Ho) continue;            // the convolution's zero padding (uniform over the block)
      int y0, y1; float ly;
      src_index2(ry, py, Hi, y0, y1, ly);
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const float w = half ? ly : 1.f - ly;
        if (w == 0.f) continue;                    // uniform
        const int rowoff = (half ? y1 : y0) * Wi * pix + 3 * r * N;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            float v[VEC];
            V::ld(zb, rowoff + coff[kx] + s * N, v);
#pragma unroll
            for (int e = 0; e < VEC; ++e) h[s][kx][e] += w * v[e];
          }
        }
      }
    }
    float o[F][VEC];
#pragma unroll
    for (int j = 0; j < F; ++j) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[j][e] = 0.f;
#pragma unroll
      for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int e = 0; e < VEC; ++e) o[j][e] += wx[j + s][kx] * h[s][kx][e];
    }
#pragma unroll
    for (int cc = 0; cc < CELLS; ++cc) {
      if (cell == cc) {                            // uniform: keeps the accumulator indices compile-time constants
#pragma unroll
        for (int j = 0; j < F; ++j)
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[cc * F + j][e] += o[j][e];
      }
    }
  }
}

// grid = (ceil(Wo / RUN * N / VEC / 256), B * Ho); addvec (f32 [N], may be null) is added to every output (conv bias, or
// the folded BatchNorm shift in eval mode), then the optional ReLU.
template <typename V, int VEC, int RUN>
__global__ __launch_bounds__(256) void resize_conv3x3_fwd_sum_kernel(TapSrc src, int nsrc, int N, void* out, int Ho, int Wo,
                                                                     const float* __restrict__ addvec, int relu) {
  const int cv = N / VEC;
  const int nblk = gridDim.x * gridDim.y;
  const int id = blockIdx.y * gridDim.x + blockIdx.x;
  const int q8 = nblk >> 3, r8 = nblk & 7, xcd = id & 7, idx = id >> 3;      // XCD-major: neighbouring rows share an L2
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  const int brow = lid / gridDim.x, bx = lid - brow * gridDim.x;
  const int j0 = bx * 256 + threadIdx.x;
  if (j0 >= (Wo / RUN) * cv) return;
  const int b = brow / Ho, oy = brow - b * Ho;
  const int xr = j0 / cv, c = (j0 - xr * cv) * VEC;
  const int ox0 = xr * RUN;
  float acc[RUN][VEC];
#pragma unroll
  for (int p = 0; p < RUN; ++p)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[p][e] = 0.f;
  for (int k = 0; k < nsrc; ++k) {
    const int F = src.F[k];
    if constexpr (RUN >= 8) { if (F == 8) tapsum_source<V, VEC, RUN, 8>(acc, src.p[k], src.H[k], src.W[k], N, b, oy, Ho, ox0, Wo, c); }
    if constexpr (RUN >= 4) { if (F == 4) tapsum_source<V, VEC, RUN, 4>(acc, src.p[k], src.H[k], src.W[k], N, b, oy, Ho, ox0, Wo, c); }
    if (F == 2) tapsum_source<V, VEC, RUN, 2>(acc, src.p[k], src.H[k], src.W[k], N, b, oy, Ho, ox0, Wo, c);
  }
  float add[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) add[e] = addvec ? addvec[c + e] : 0.f;
  const int64_t obase = (((int64_t)b * Ho + oy) * Wo + ox0) * N + c;
#pragma unroll
  for (int p = 0; p < RUN; ++p) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      acc[p][e] += add[e];
      if (relu) acc[p][e] = fmaxf(acc[p][e], 0.f);
    }
    V::st(out, obase + (int64_t)p * N, acc[p]);
  }
}

// ---- the same sum on the matrix cores (bf16, N % 64 == 0): the production form.
// The pixel-by-pixel kernel above reads every z vector ~24 times through L1/L2 (13.5 x the output bytes: measured 1.5 ms for the
// neck's x4 level against 0.3 ms of HBM time).  Per 4 x 4 output patch the sum is a small dense product that is THE SAME for
// every channel:   out[p, n] = sum_k A[p, k] z[k, n],   k = (filter tap (r, s), window pixel (wy, dx)),
// where the window is the 3 x 3 (factor 2: 4 x 4) low-resolution pixels the patch's 6 x 6 tap positions interpolate from and
// A[p, k] = Uy[oy + r - 1, wy] * Ux[ox + s - 1, dx] (zero outside the output = the convolution's padding).  A factorises, so k
// is laid out as a = (r, wy) outer, b = (s, dx) inner padded to 16: K = 16 * 3 WIN, five or six v_mfma_f32_16x16x32_bf16
// steps per 16 channels.  The weights are bilinear fractions (k/4, k/8, k/16 and their pairwise products): exact in bf16.
// A block = 4 output rows x 4 PXB columns x 64 channels of one image: it stages the low-resolution window (rows of 64
// channels = 128 B, every (pixel, tap) one row) by LDS-DMA as it lies in memory, builds the two 1-D weight tables in LDS,
// and each wave runs its patches: z fragments (rows = channels) through ds_read_b64_tr_b16, weight fragments (columns =
// pixels) from the tables.  Sources are staged one after the other into the same LDS and accumulate in registers; the
// result leaves through an LDS transpose as whole 128-byte lines.  f32 accumulation, fixed order.
// (The LDS row types, the row swizzle tm_swz and the DMA's out-of-range offset kTmOob: resample_vec.h, shared with the backward.)
struct TapMArgs {
  const uint16_t* z[3];
  int H[3], W[3], LF[3];          // low-resolution size and log2(factor) of every source
  int nsrc, N, Ho, Wo, B;
  uint16_t* out;
  const float* addvec;
  int relu;
  int nslots, slot_off[3];        // version 2: byte offsets of the window slots (two for one source, else one per source)
  int gx, nblk;                   // version 2 (persistent): patches per output row block, patches in all
};

// the two 1-D weight tables of source k for the block at (oy0, oxb0): TYs [4][12] (+ padding to 64 floats), TXs [COLS][16]
template <int PXB, int LF>
__device__ __forceinline__ void tapm_tables(const TapMArgs& a, int k, float* TYs, float* TXs, int oy0, int oxb0, int tid) {
  constexpr int WIN = LF == 1 ? 4 : 3, lf = LF;
  constexpr int COLS = 4 * PXB, NA = 3 * WIN;
  const int Hi = a.H[k], Wi = a.W[k];
  const int wr0 = (oy0 >> lf) - 1;
  const float ry = (float)Hi / (float)a.Ho, rx = (float)Wi / (float)a.Wo;
  if (tid < 48) {
    const int py = tid / 12, ai = tid - py * 12;
    float w = 0.f;
    if (ai < NA) {
      const int r = ai / WIN, wy = ai - r * WIN, pos = oy0 + py + r - 1;
      if (pos >= 0 && pos < a.Ho) {
        int y0, y1; float ly;
        src_index2(ry, pos, Hi, y0, y1, ly);
        const int row = wr0 + wy;
        w = (y0 == row ? 1.f - ly : 0.f) + (y1 == row ? ly : 0.f);
      }
    }
    TYs[tid] = w;
  }
  for (int i = tid; i < COLS * 16; i += 256) {
    const int pc = i >> 4, bi = i & 15;
    float w = 0.f;
    if (bi < NA) {
      const int s3 = bi / WIN, dx = bi - s3 * WIN, pos = oxb0 + pc + s3 - 1;
      if (pos >= 0 && pos < a.Wo) {
        int x0, x1; float lx;
        src_index2(rx, pos, Wi, x0, x1, lx);
        const int col = ((oxb0 + (pc & ~3)) >> lf) - 1 + dx;          // the PATCH's window starts at its own first cell - 1
        w = (x0 == col ? 1.f - lx : 0.f) + (x1 == col ? lx : 0.f);
      }
    }
    TXs[i] = w;
  }
}

// stage the window of source k, channels c0 .. c0 + 63: LDS row R = (wyi * WC + wci) * 9 + tap, 128 bytes; no wait
template <int PXB, int LF>
__device__ __forceinline__ void tapm_issue(const TapMArgs& a, int k, unsigned lds_stage, int b, int oy0, int oxb0, int c0, int lane,
                                           int wave) {
  constexpr int WIN = LF == 1 ? 4 : 3, lf = LF;
  constexpr int COLS = 4 * PXB;
  const int Hi = a.H[k], Wi = a.W[k], N = a.N;
  constexpr int WC = ((COLS - 4) >> lf) + WIN;        // window columns of the block (compile-time: the divisions below are cheap)
  const int wr0 = (oy0 >> lf) - 1, wcb0 = (oxb0 >> lf) - 1;
  const srd_t srd = make_srd(a.z[k] + (int64_t)b * Hi * Wi * 9 * N, (unsigned)((int64_t)Hi * Wi * 9 * N * 2));
  constexpr int nrows = WIN * WC * 9, npieces = (nrows + 7) >> 3;
  for (int piece = wave; piece < npieces; piece += 4) {
    const int R = piece * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ tm_swz(R);
    const int pc = R / 9, t = R - pc * 9;
    const int wyi = pc / WC, wci = pc - wyi * WC;
    const int row = wr0 + wyi, col = wcb0 + wci;
    const bool ok = R < nrows && row >= 0 && row < Hi && col >= 0 && col < Wi;
    const unsigned v = ok ? (unsigned)((((row * Wi + col) * 9 + t) * N + c0) * 2 + chunk * 16) : kTmOob;
    dma16_buf(v, srd, 0u, lds_stage + piece * 1024);
  }
}

// the wave's patches of source k from a staged window: acc[j2][nt] += z-fragments x weight-fragments
template <int PXB, int LF>
__device__ __forceinline__ void tapm_mfma(const TapMArgs& a, int k, f32x4_t (&acc)[PXB / 4][4], const float* TYs, const float* TXs,
                                          const unsigned char* stage, int lane, int wave) {
  constexpr int WIN = LF == 1 ? 4 : 3, lf = LF;
  constexpr int COLS = 4 * PXB, NA = 3 * WIN, NKS = (NA + 1) / 2;
  constexpr int WC = ((COLS - 4) >> lf) + WIN;
  int lane_mfma = lane;
  asm volatile("" : "+v"(lane_mfma));                 // keeps the fragment address arithmetic below this point (register budget)
  const int L = lane_mfma & 15, g = lane_mfma >> 4;
#pragma unroll
  for (int j2 = 0; j2 < PXB / 4; ++j2) {
    const int j = wave + 4 * j2;
    const int wcj = (4 * j) >> lf;                                    // the patch's window start inside the block's window
    // weight fragments (B operand: column = pixel L of the patch, k = 16 a + b)
    float txv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) txv[e] = TXs[(4 * j + (L & 3)) * 16 + 8 * (g & 1) + e];
    bf16x8_t wf[NKS];
    int raddr[NKS][2];                                                // LDS byte offset of this lane's 8-byte piece for channel tile 0
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int ai = 2 * ks + (g >> 1);
      const float ty = TYs[(L >> 2) * 12 + ai];                       // zero for ai >= NA (table padding)
      uint32_t pk[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) pk[e] = pack_bf16x2(ty * txv[2 * e], ty * txv[2 * e + 1]);
      wf[ks] = __builtin_bit_cast(bf16x8_t, make_uint4(pk[0], pk[1], pk[2], pk[3]));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int bq = 8 * (g & 1) + 4 * h + (L >> 2);
        const bool ok = ai < NA && bq < NA;
        const int r = ai / WIN, wy = ai - r * WIN, s3 = bq / WIN, dx = bq - s3 * WIN;
        const int R = ok ? ((wy * WC + wcj + dx) * 9 + 3 * r + s3) : 0;   // padding slots: any staged row, their weight is zero
        // 16-byte slot = (channel >> 3) ^ swizzle(R); channel = 16 nt + 4 (L & 3): nt only flips slot bits 1-2 -> one XOR per tile
        raddr[ks][h] = R * 128 + (((((L & 3) >> 1) ^ tm_swz(R))) << 4) + (L & 1) * 8;
      }
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const tm_s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tm_lds_s16x4_ptr)(stage + (raddr[ks][0] ^ (nt << 5))));
        const tm_s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tm_lds_s16x4_ptr)(stage + (raddr[ks][1] ^ (nt << 5))));
        const tm_s16x8_t zv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[j2][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, zv), wf[ks], acc[j2][nt], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);          // one channel tile's fragment reads in flight at a time (register budget)
    }
  }
}

// accumulators -> (+ addvec, ReLU) -> bf16 -> LDS tile [4 rows][COLS pixels] x 128 B, 16-byte slots swizzled by pixel
template <int PXB>
__device__ __forceinline__ void tapm_to_tile(const TapMArgs& a, f32x4_t (&acc)[PXB / 4][4], unsigned char* tile, int c0, int lane, int wave) {
  constexpr int COLS = 4 * PXB;
  const int L = lane & 15, g = lane >> 4;
#pragma unroll
  for (int j2 = 0; j2 < PXB / 4; ++j2) {
    const int pp = (L >> 2) * COLS + 4 * (wave + 4 * j2) + (L & 3);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int ch = 16 * nt + 4 * g;
      float v[4];
      const float4 av = a.addvec ? *(const float4*)(a.addvec + c0 + ch) : make_float4(0.f, 0.f, 0.f, 0.f);   // (c0 + ch) % 4 == 0
      const float add[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = acc[j2][nt][i] + add[i];
        if (a.relu) v[i] = fmaxf(v[i], 0.f);
      }
      *(uint2*)(tile + pp * 128 + ((((ch >> 3) ^ (pp & 7))) << 4) + (ch & 7) * 2) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
  }
}

// grid = (ceil(Wo / (4 PXB)) * N / 64, B * ceil(Ho / 4)); dynamic LDS = 256 + 256 PXB + max over the sources of the window bytes
template <int PXB>
__global__ __launch_bounds__(256, PXB == 8 ? 3 : 4) void resize_conv3x3_fwd_sum_mfma_kernel(const TapMArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int COLS = 4 * PXB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nchunks = a.N >> 6, nprow = (a.Ho + 3) >> 2;
  const int nblk = gridDim.x * gridDim.y;
  const int id = blockIdx.y * gridDim.x + blockIdx.x;
  const int q8 = nblk >> 3, r8 = nblk & 7, xcd = id & 7, idx = id >> 3;      // XCD-major: neighbouring patch rows share an L2
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  const int brow = lid / gridDim.x, bx = lid - brow * gridDim.x;
  const int b = brow / nprow, oy0 = (brow - b * nprow) * 4;
  const int cb = bx / nchunks, c0 = (bx - cb * nchunks) * 64, oxb0 = cb * COLS;
  float* TYs = (float*)smem;
  float* TXs = TYs + 64;
  unsigned char* stage = smem + 256 + COLS * 64;
  const unsigned lds_stage = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) void*)stage);
  f32x4_t acc[PXB / 4][4];
#pragma unroll
  for (int j2 = 0; j2 < PXB / 4; ++j2)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[j2][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < a.nsrc; ++k) {
    if (k > 0) __syncthreads();                       // the previous source's fragment reads are done: tables and window are rewritten
    if (a.LF[k] == 1) { tapm_tables<PXB, 1>(a, k, TYs, TXs, oy0, oxb0, tid); tapm_issue<PXB, 1>(a, k, lds_stage, b, oy0, oxb0, c0, lane, wave); }
    else if (a.LF[k] == 2) { tapm_tables<PXB, 2>(a, k, TYs, TXs, oy0, oxb0, tid); tapm_issue<PXB, 2>(a, k, lds_stage, b, oy0, oxb0, c0, lane, wave); }
    else { tapm_tables<PXB, 3>(a, k, TYs, TXs, oy0, oxb0, tid); tapm_issue<PXB, 3>(a, k, lds_stage, b, oy0, oxb0, c0, lane, wave); }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (a.LF[k] == 1) tapm_mfma<PXB, 1>(a, k, acc, TYs, TXs, stage, lane, wave);
    else if (a.LF[k] == 2) tapm_mfma<PXB, 2>(a, k, acc, TYs, TXs, stage, lane, wave);
    else tapm_mfma<PXB, 3>(a, k, acc, TYs, TXs, stage, lane, wave);
  }
  __syncthreads();
  // ---- epilogue through an LDS transpose (the window's memory is free now)
  unsigned char* tile = stage;
  tapm_to_tile<PXB>(a, acc, tile, c0, lane, wave);
  __syncthreads();
  for (int i = tid; i < 4 * COLS * 8; i += 256) {
    const int pp = i >> 3, chunk = i & 7;
    const int py = pp / COLS, oy = oy0 + py, ox = oxb0 + pp - py * COLS;
    if (oy < a.Ho && ox < a.Wo) {
      const uint4 v = *(const uint4*)(tile + pp * 128 + ((chunk ^ (pp & 7)) << 4));
      *(uint4*)(a.out + (((int64_t)b * a.Ho + oy) * a.Wo + ox) * a.N + c0 + chunk * 8) = v;
    }
  }
}

// ---- what versions 2 and 3 share: the output tile, and the counted waits of their steady state.
// A step's outputs leave through an LDS tile of 4 rows x `cols` pixels x 64 bf16 channels (128 bytes), 16 bytes per thread and store.
constexpr int tap_tile_bytes(int cols) { return 4 * cols * 128; }
// the low-resolution window of a 4 x cols block of a factor-2^lf source; the staging loops write whole 1 KiB pieces (8 rows): rounded up to that
constexpr int tap_window_bytes(int cols, int lf) { return ((lf == 1 ? 4 : 3) * (((cols - 4) >> lf) + (lf == 1 ? 4 : 3)) * 9 * 128 + 1023) / 1024 * 1024; }
constexpr int kTapTileBytes = tap_tile_bytes(16);          // version 3 (and version 2 at PXB = 4): 4 x 16 pixels
constexpr int tap_stores_per_flush(int tile_bytes, int threads) { return tile_bytes / (threads * 16); }
constexpr int kTapM2Threads = 256, kRollThreads = 256, kRoll3Threads = 512;   // workgroup sizes: launch bounds, store loops, launcher
// The vmcnt immediate that leaves everything younger than a step's fetch in flight (the vm counter retires in order, LDS-DMA
// fetches and stores alike): with the fetches running `depth` steps ahead, the fetch that is waited for was followed by the
// stores of one flush and then depth - 1 times by a fetch and a flush.  The arguments are the constants the fetch and store
// loops run over: an edit to either side moves the immediate with it.
constexpr int steady_vmcnt(int depth, int dma_per_step, int stores_per_step) {
  return stores_per_step + (depth - 1) * (dma_per_step + stores_per_step);
}
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vmcnt_lgkm0() {       // (why lgkmcnt(0) rides along: see resize_conv3x3_fwd_sum_roll_kernel)
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

// ---- version 2: one block owns its 4 x 4 PXB output pixels for ALL channels and walks the 64-channel chunks (and, per chunk,
// the sources) through LDS window slots: the window of step i + 1 is in flight while step i runs on the matrix cores.
// Everything that does not depend on the channel is computed ONCE per block and kept in registers: the weight fragments
// and fragment addresses of the wave's patches, and the per-lane DMA offsets (the chunk enters as the buffer instruction's
// scalar offset).  PMC of version 1 on the neck's x4 level: 1400 VALU instructions per wave and 64-channel block -- runtime
// divisions in the DMA addressing, the table and fragment set-up -- against 40 MFMAs: VALU-bound at 2.2 TB/s.
// With `stats` the per-channel sum and sum of squares of the (bf16-rounded) outputs of the block are written as one partial
// row each ([block][2][N] f32, the layout bn_stats_final reduces): train-mode BatchNorm needs no statistics pass.
// grid = (ceil(Wo / (4 PXB)), B * ceil(Ho / 4)); dynamic LDS = NSRC * (256 + 256 PXB) tables + 512 PXB tile bytes + the window
// slots: one source -> two slots used alternately; several sources -> one slot per source (step (chunk, k) reads slot k while
// the next step's window lands in another one)
// LF0 (single source only): the factor as a template parameter -- the fragment count per channel tile, the DMA piece count and
// the window slot then need no run-time branches (0 = read a.LF[k] at run time)
template <int PXB, int NSRC, int LF0 = 0>
__global__ __launch_bounds__(kTapM2Threads, NSRC == 1 ? 3 : 1) void resize_conv3x3_fwd_sum_mfma2_kernel(const TapMArgs a, float* stats) {
  static_assert(LF0 == 0 || NSRC == 1, "compile-time factor: one source");
  auto lf_of = [&](int k) { return LF0 ? LF0 : a.LF[k]; };
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int COLS = 4 * PXB, TBL = 256 + COLS * 64, NPW = PXB / 4;
  constexpr int MAXP = PXB == 8 ? 9 : 12;                 // DMA pieces per wave and window (factor 2 needs 4 x 16 blocks)
  constexpr int TILE = tap_tile_bytes(COLS);
  constexpr int STORES = tap_stores_per_flush(TILE, kTapM2Threads);   // output stores per thread and chunk (PXB / 2)
  static_assert(STORES * kTapM2Threads * 16 == TILE, "version 2: the tile is exactly threads * stores * 16 bytes");
  constexpr int AHEAD = 1;                                 // steps the window fetches run ahead: issue(it + AHEAD) while step it computes
  static_assert(AHEAD == 1, "version 2: one step ahead, so only stores are younger than the fetch that is waited for; the fetches "
                            "are not padded (their count differs between the waves) and must not enter the wait");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nchunks = a.N >> 6, nprow = (a.Ho + 3) >> 2;
  const int nblk = a.nblk;
  unsigned char* tile = smem + NSRC * TBL;
  unsigned char* ring = tile + TILE;
  const unsigned lds_ring = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) void*)ring);
  const int L = lane & 15, g = lane >> 4;
  bf16x8_t wf[NSRC][NPW][6];                              // weight fragments (B operand: column = pixel L of the patch)
  int raddr[NSRC][NPW][6][2];                             // LDS byte offsets of the z fragment pieces, channel tile 0
  unsigned doff[NSRC][MAXP];                              // DMA source offsets of this lane's pieces (channel 0), for the patch at (set_wr0, set_wc0)
  srd_t srd[NSRC];
  // PERSISTENT (round 4): a workgroup walks patches vid = blockIdx.x, + gridDim.x, ...  Everything channel-independent -- the
  // two weight tables, the weight fragments, the fragment and DMA offsets: ~6000 VALU instructions per wave with their runtime
  // divisions, as much as 26 of the 12 channel steps of a 768-channel patch (PMC: 366 M VALU instructions per launch of which
  // 115 M in the channel loop) -- is the SAME for every patch whose windows lie inside the image and whose rows have the same
  // interpolation phase: there only the buffer descriptor moves (by the distance between the patch positions), and the set-up
  // runs again only for patches that touch the image border or change phase (key < 0 / key differs).
  int set_key = -2, set_wr0[NSRC], set_wc0[NSRC];
#pragma unroll
  for (int k = 0; k < NSRC; ++k) { set_wr0[k] = 0; set_wc0[k] = 0; }
  for (int vid = blockIdx.x; vid < nblk; vid += gridDim.x) {
  const int q8 = nblk >> 3, r8 = nblk & 7, xcd = vid & 7, idx = vid >> 3;      // XCD-major: neighbouring patch rows share an L2
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  const int brow = lid / a.gx, cb = lid - brow * a.gx;
  const int b = brow / nprow, oy0 = (brow - b * nprow) * 4;
  const int oxb0 = cb * COLS;
  const bool full = oy0 + 4 <= a.Ho && oxb0 + COLS <= a.Wo;
  int key = full ? 0 : -1;
#pragma unroll
  for (int k = 0; k < NSRC; ++k) {
    const int lf = lf_of(k), win = lf == 1 ? 4 : 3, WC = ((COLS - 4) >> lf) + win;
    const int wr0 = (oy0 >> lf) - 1, wc0 = (oxb0 >> lf) - 1;
    if (wr0 < 0 || wc0 < 0 || wr0 + win > a.H[k] || wc0 + WC > a.W[k]) key = -1;
    else if (key >= 0) key = key * 8 + (oy0 & ((1 << lf) - 1));      // row phase (4-row patches: only factor 8 has two); columns: 16 | oxb0
  }
  if (key < 0 || key != set_key) {
  set_key = key;
  if (vid != (int)blockIdx.x) __syncthreads();            // the previous patch's fragment set-up / statistics may still read the tables
  // (the set-up derives everything from an opaque copy of the thread id: otherwise its lane-only subexpressions are hoisted in
  // front of the patch loop and stay live -- spilled -- across the channel loop)
  int tid_s = tid;
  asm volatile("" : "+v"(tid_s));
  const int lane = tid_s & 63, L = lane & 15, g = lane >> 4;
#pragma unroll
  for (int k = 0; k < NSRC; ++k) {
    float* TYs = (float*)(smem + k * TBL);
    if (lf_of(k) == 1) tapm_tables<PXB, 1>(a, k, TYs, TYs + 64, oy0, oxb0, tid_s);
    else if (lf_of(k) == 2) tapm_tables<PXB, 2>(a, k, TYs, TYs + 64, oy0, oxb0, tid_s);
    else tapm_tables<PXB, 3>(a, k, TYs, TYs + 64, oy0, oxb0, tid_s);
  }
  __syncthreads();
  // ---- channel-independent state of every source
#pragma unroll
  for (int k = 0; k < NSRC; ++k) {
    const int lf = lf_of(k), Hi = a.H[k], Wi = a.W[k];
    const bool w4 = lf == 1;
    const int win = w4 ? 4 : 3, na = 3 * win;
    const int WC = ((COLS - 4) >> lf) + win;
    const float* TYs = (const float*)(smem + k * TBL);
    const float* TXs = TYs + 64;
#pragma unroll
    for (int j2 = 0; j2 < NPW; ++j2) {
      const int j = wave + 4 * j2;
      const int wcj = (4 * j) >> lf;
      float txv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) txv[e] = TXs[(4 * j + (L & 3)) * 16 + 8 * (g & 1) + e];
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) {
        const int ai = 2 * ks + (g >> 1);
        const float ty = TYs[(L >> 2) * 12 + ai];         // zero for ai >= na (table padding)
        uint32_t pk[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) pk[e] = pack_bf16x2(ty * txv[2 * e], ty * txv[2 * e + 1]);
        wf[k][j2][ks] = __builtin_bit_cast(bf16x8_t, make_uint4(pk[0], pk[1], pk[2], pk[3]));
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int bq = 8 * (g & 1) + 4 * h + (L >> 2);
          const bool ok = ai < na && bq < na;
          const int r = w4 ? ai >> 2 : ai / 3, wy = ai - r * win, s3 = w4 ? bq >> 2 : bq / 3, dx = bq - s3 * win;
          const int R = ok ? ((wy * WC + wcj + dx) * 9 + 3 * r + s3) : 0;
          raddr[k][j2][ks][h] = R * 128 + (((((L & 3) >> 1) ^ tm_swz(R))) << 4) + (L & 1) * 8;
        }
      }
    }
    const int wr0 = (oy0 >> lf) - 1, wcb0 = (oxb0 >> lf) - 1;
    set_wr0[k] = wr0; set_wc0[k] = wcb0;
    const int nrows = win * WC * 9;
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
      const int piece = wave + 4 * i;
      const int R = piece * 8 + (lane >> 3);
      const int chunk = (lane & 7) ^ tm_swz(R);
      const int pc = R / 9, t = R - pc * 9;
      const int wyi = pc / WC, wci = pc - wyi * WC;
      const int row = wr0 + wyi, col = wcb0 + wci;
      const bool ok = R < nrows && row >= 0 && row < Hi && col >= 0 && col < Wi;
      doff[k][i] = ok ? (unsigned)((((row * Wi + col) * 9 + t) * a.N) * 2 + chunk * 16) : kTmOob;
    }
  }
  }
  // the image's buffer descriptor, moved from the set-up patch to this one (interior patches only: every piece stays inside)
#pragma unroll
  for (int k = 0; k < NSRC; ++k) {
    const int lf = lf_of(k), Hi = a.H[k], Wi = a.W[k];
    const int64_t shift = ((int64_t)(((oy0 >> lf) - 1) - set_wr0[k]) * Wi + (((oxb0 >> lf) - 1) - set_wc0[k])) * 9 * a.N;
    srd[k] = make_srd(a.z[k] + (int64_t)b * Hi * Wi * 9 * a.N + shift, (unsigned)((int64_t)Hi * Wi * 9 * a.N * 2));
  }
  auto issue = [&](int it) {
    const int c = it / NSRC, k = it - c * NSRC;
    const unsigned dst = lds_ring + (NSRC == 1 ? (it & 1) * a.slot_off[1] : a.slot_off[it % a.nslots]);   // one source: two slots, slot_off[0] = 0
#pragma unroll
    for (int kk = 0; kk < NSRC; ++kk) {
      if (kk != k) continue;                               // (static source index for the register arrays)
      const int lf = lf_of(kk), win = lf == 1 ? 4 : 3;
      const int npieces = (win * (((COLS - 4) >> lf) + win) * 9 + 7) >> 3;
#pragma unroll
      for (int i = 0; i < MAXP; ++i) {
        if (wave + 4 * i < npieces) dma16_buf(doff[kk][i], srd[kk], (unsigned)(c * 128), dst + (wave + 4 * i) * 1024);
      }
    }
  };
  f32x4_t acc[NPW][4];
#pragma unroll
  for (int j2 = 0; j2 < NPW; ++j2)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[j2][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int nit = nchunks * NSRC;
  issue(0);
  for (int it = 0; it < nit; ++it) {
    const int c = it / NSRC, k = it - c * NSRC;
    // this wave's pieces of step `it` have landed.  They were issued BEFORE the previous step's output stores, and vmcnt
    // retires in order: inside the image (every thread stores exactly STORES pieces per chunk) the wait leaves those stores
    // in flight instead of exposing their acknowledgement.  The fetches run one step ahead, so nothing else is younger.
    if (full && it > 0 && (it - 1) % NSRC == NSRC - 1) {
      if (stats && wave < 2) wait_vmcnt<steady_vmcnt(AHEAD, 0, STORES + 1)>();   // (waves 0 and 1 also wrote one statistics row each)
      else wait_vmcnt<steady_vmcnt(AHEAD, 0, STORES)>();
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();                                      // ... everyone's; nobody reads the other slot or the tile any more
    if (it + AHEAD < nit) issue(it + AHEAD);
    const unsigned char* stage = ring + (NSRC == 1 ? (it & 1) * a.slot_off[1] : a.slot_off[it % a.nslots]);
#pragma unroll
    for (int kk = 0; kk < NSRC; ++kk) {
      if (kk != k) continue;
      const int nks = lf_of(kk) == 1 ? 6 : 5;
#pragma unroll
      for (int j2 = 0; j2 < NPW; ++j2) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
          for (int ks = 0; ks < 6; ++ks) {
            if (ks < nks) {
              const tm_s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tm_lds_s16x4_ptr)(stage + (raddr[kk][j2][ks][0] ^ (nt << 5))));
              const tm_s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tm_lds_s16x4_ptr)(stage + (raddr[kk][j2][ks][1] ^ (nt << 5))));
              const tm_s16x8_t zv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
              acc[j2][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, zv), wf[kk][j2][ks], acc[j2][nt], 0, 0, 0);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    if (k != NSRC - 1) continue;
    // ---- the chunk is complete: transpose through the tile, store whole 128-byte lines, optional statistics
    const int c0 = c * 64;
    tapm_to_tile<PXB>(a, acc, tile, c0, lane, wave);
#pragma unroll
    for (int j2 = 0; j2 < NPW; ++j2)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[j2][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    float s1[8], s2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
#pragma unroll
    for (int u = 0; u < STORES; ++u) {
      const int i = tid + kTapM2Threads * u;
      const int pp = i >> 3, chunk = i & 7;                // chunk = tid & 7 for every u: a thread always owns the same 8 channels
      const int py = pp / COLS, oy = oy0 + py, ox = oxb0 + pp - py * COLS;
      if (full || (oy < a.Ho && ox < a.Wo)) {               // `full` is uniform: then every thread stores, and the wait above counts on it
        const uint4 v = *(const uint4*)(tile + pp * 128 + ((chunk ^ (pp & 7)) << 4));
        *(uint4*)(a.out + (((int64_t)b * a.Ho + oy) * a.Wo + ox) * a.N + c0 + chunk * 8) = v;
        if (stats) {
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = __uint_as_float(w[e] << 16), hi = __uint_as_float(w[e] & 0xffff0000u);
            s1[2 * e] += lo; s2[2 * e] += lo * lo;
            s1[2 * e + 1] += hi; s2[2 * e + 1] += hi * hi;
          }
        }
      }
    }
    if (stats) {
      // lanes with equal (lane & 7) own the same channels: fold lane bits 3, 4, 5, then the four waves through the (by then
      // idle) tile memory, in a fixed order
#pragma unroll
      for (int e = 0; e < 8; ++e) {
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) { s1[e] += __shfl_xor(s1[e], o, 64); s2[e] += __shfl_xor(s2[e], o, 64); }
      }
      __syncthreads();                                    // every thread has read its pixels from the tile
      float* red = (float*)tile;                          // [wave][sum | sum of squares][64 channels]
      if (lane < 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { red[(wave * 2) * 64 + lane * 8 + e] = s1[e]; red[(wave * 2 + 1) * 64 + lane * 8 + e] = s2[e]; }
      }
      __syncthreads();
      if (tid < 128) {                                     // waves 0 and 1: the `+ 1` of their wait
        const int which = tid >> 6, ch = tid & 63;
        const float t = ((red[(0 * 2 + which) * 64 + ch] + red[(1 * 2 + which) * 64 + ch]) + red[(2 * 2 + which) * 64 + ch]) +
                        red[(3 * 2 + which) * 64 + ch];
        stats[((int64_t)lid * 2 + which) * a.N + c0 + ch] = t;
      }
    }
  }
  __syncthreads();                                        // the next patch's first window overwrites slot 0, its statistics the tile
  }
}

// ---- version 3 (round 6): sources of factor 2 / 4 (one source, Ho % 4 == 0) or 2 + 4 + 8 (UperNet's fpn_bottleneck, Ho % 8 == 0)
// -- a ROLLING window of low-resolution rows.
// Versions 1 and 2 stage the whole 3 (4) x WC pixel window of every 4 x 16 patch: each tap-product pixel travels L2 -> LDS 4.5 times
// (factor 4) and, because the patches that share it run at different times, 2.4 times from memory (PMC: 1383 MB fetched per
// launch for 574 MB of tap products at batch 32) -- the kernel moved its over-fetched bytes at 4.5 TB/s and was memory-bound on them.
// Here a workgroup owns a COLUMN = (image, 64-channel chunk, strip of 16 output columns) and walks it top to bottom, four
// output rows per step: the window rows live in a ring of LDS row slots and only the new low-resolution rows of a later step
// are fetched (D steps ahead, by LDS-DMA).  The strips of one (image, chunk) are walked by neighbouring workgroups of ONE XCD
// at the same pace, so the one or two window columns two strips share come out of that L2.
// What makes one set-up per workgroup enough (a strip's columns all look alike):
//   * rows outside the image are CLAMPED in the DMA address instead of re-weighted: torch's clamp of the source index is the
//     same as bilinear weights on an edge-replicated map ((1 - l) z[0] + l z[0] = z[0], exact in f32), so the row weights
//     of every step are the interior ones;
//   * the convolution's zero padding touches the first and the last step only (tap row -1 of output row 0, tap row Ho of
//     output row Ho - 1): those two steps use weight fragments with these products zeroed (kept beside the interior ones).
// The K dimension is PACKED: k = (tap row, window row) * NA + (tap column, window column), NA = 3 WIN, K = NA^2 = 81 (144 for
// factor 2) in 3 (5) steps of 32 -- versions 1 / 2 pad the inner index to 16 (5 and 6 steps).  Compute was the bound of the
// first form of this kernel (fpn_bottleneck: 809 us of matrix-core + LDS work against 608 us for all its memory traffic).
// A step's output leaves through the LDS tile at the TOP of the next step and has the whole step to be acknowledged.
// D = steps the row fetches run ahead.  One step ahead leaves a workgroup one memory latency per step (factor 4, four workgroups
// per CU: 4.1 us per step and workgroup, 3.1 TB/s); D > 1: the wait at the top of a step leaves the later fetches -- and the
// stores between them; every wave issues the same number in a strip that lies inside the image -- in flight (vmcnt retires in
// order).
// STATS (one source): per-channel sum and sum of squares of the bf16-rounded outputs on the matrix cores, straight from the
// tile: with the tile fragment F (K = 32 pixels x 16 channels) as BOTH operands the diagonal of F^T F is the sum of squares,
// ones^T F the sum; the accumulators run over the whole column, so a launch writes B * strips partial rows (version 2: one per
// patch = 36 x as many, reduced by shuffles and two extra barriers per step: 1510 us with statistics against 1082 us without
// at batch 64).
// Three sources: one ring per source and one set of accumulators.  Factor 8: a step of four output rows is half a cell -- two
// row phases with their own weight fragments, a new window row every other step.  One workgroup per CU (the three rings are
// 96 + 35 + 20 KiB at D = 2); pieces a wave does not have, and the factor-8 source's idle steps, are fetches whose lanes are all
// out of range (zeros into a spare KiB, no memory traffic), so one vmcnt immediate serves every wave and step.
template <int LF, int D, int NW = 4>                       // NW: waves of the workgroup (4: a wave owns a patch; 8: a patch and half of its channel tiles)
struct RollSrc {
  static constexpr int WIN = LF == 1 ? 4 : 3, NPH = LF == 3 ? 2 : 1;
  static constexpr int NA = 3 * WIN, KR = NA * NA, NKS = (KR + 31) / 32;
  static constexpr int WC = (12 >> LF) + WIN, ROWS = WC * 9, PIECES = (ROWS + 7) / 8, SLOT = PIECES * 1024;
  static constexpr int RPS = LF == 1 ? 2 : 1;              // new window rows of a step that fetches
  static constexpr int NSLOT = WIN + (LF == 3 ? (D + 1) / 2 : D * RPS);
  static constexpr int MAXP = (PIECES + NW - 1) / NW, NDMA = RPS * MAXP, BYTES = NSLOT * SLOT;   // NDMA: DMA instructions of a padded fetching step
  static constexpr int NWAVES = NW;
  static constexpr int NMW = (NKS + 3) / 4;
  static_assert(LF != 3 || RPS == 1, "factor 8: a step fetches one row or (every other step) none; the idle step pads one row's worth");
  bf16x8_t wf[NPH][NKS];                                   // weight fragments (B operand: column = pixel of the patch)
  unsigned mtop[NMW], mbot[NMW];                           // bit 8 (ks % 4) + e of word ks / 4: element e of K-step ks is zero in the first / last step
  unsigned araddr[NKS][2];                                 // ring-relative byte offset of the lane's two fragment pieces, window row 0 of the step in slot 0
  unsigned doff[MAXP];
  srd_t srd;
  unsigned lds;                                            // LDS address of the ring
  int Hi;
  int64_t row_bytes;

  // the weight tables live in `tab` (>= 128 + 256 floats) during the call; two barriers inside
  __device__ __forceinline__ void setup(float* tab, unsigned lds_ring, int Hi_, int Wi, int Wo, int N, int oxb0, int tid, int wave) {
    const int lane = tid & 63, L = lane & 15, g = lane >> 4;
    Hi = Hi_;
    lds = lds_ring;
    row_bytes = (int64_t)Wi * 9 * N * 2;
    float* TY = tab;                                       // [NPH][4][12] (64 floats per phase)
    float* TX = tab + 128;                                 // [16][16]
    if (tid < 48 * NPH) {
      const int ph = tid / 48, q = tid - ph * 48, py = q / 12, ai = q - py * 12;
      float w = 0.f;
      if (ai < NA) {
        const int r = ai / WIN, wy = ai - r * WIN;
        const float s = ((float)(4 * ph + py + r - 1) + 0.5f) * (1.f / (float)(1 << LF)) - 0.5f;   // relative to the cell, not clamped
        const float fl = floorf(s);
        const int y0 = (int)fl, rr = wy - 1;
        const float ly = s - fl;
        w = (y0 == rr ? 1.f - ly : 0.f) + (y0 + 1 == rr ? ly : 0.f);
      }
      TY[ph * 64 + q] = w;
    }
    if (tid < 256) {
      const int pc = tid >> 4, bi = tid & 15;
      float w = 0.f;
      if (bi < NA) {
        const int s3 = bi / WIN, dx = bi - s3 * WIN, pos = oxb0 + pc + s3 - 1;
        if (pos >= 0 && pos < Wo) {
          int x0, x1; float lx;
          src_index2((float)Wi / (float)Wo, pos, Wi, x0, x1, lx);
          const int col = ((oxb0 + (pc & ~3)) >> LF) - 1 + dx;
          w = (x0 == col ? 1.f - lx : 0.f) + (x1 == col ? lx : 0.f);
        }
      }
      TX[tid] = w;
    }
    __syncthreads();
    const int pw = wave & 3;                               // the wave's patch
    const int wcj = (4 * pw) >> LF, wcb0 = (oxb0 >> LF) - 1;
    const int py = L >> 2, px = 4 * pw + (L & 3);
#pragma unroll
    for (int q = 0; q < NMW; ++q) { mtop[q] = 0u; mbot[q] = 0u; }
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      float wv[NPH][8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = 32 * ks + 8 * g + e;
        const bool ok = k < KR;
        const int ai = ok ? k / NA : 0, bi = ok ? k - ai * NA : 0;
        const float tx = TX[px * 16 + bi];
        const int r = ai / WIN;
#pragma unroll
        for (int ph = 0; ph < NPH; ++ph) wv[ph][e] = ok ? TY[ph * 64 + py * 12 + ai] * tx : 0.f;
        if (ok && py == 0 && r == 0) mtop[ks >> 2] |= 1u << (8 * (ks & 3) + e);      // tap row -1 of output row 0
        if (ok && py == 3 && r == 2) mbot[ks >> 2] |= 1u << (8 * (ks & 3) + e);      // tap row Ho of output row Ho - 1
      }
#pragma unroll
      for (int ph = 0; ph < NPH; ++ph)
        wf[ph][ks] = __builtin_bit_cast(bf16x8_t, make_uint4(pack_bf16x2(wv[ph][0], wv[ph][1]), pack_bf16x2(wv[ph][2], wv[ph][3]),
                                                             pack_bf16x2(wv[ph][4], wv[ph][5]), pack_bf16x2(wv[ph][6], wv[ph][7])));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = 32 * ks + 8 * g + 4 * h + (L >> 2);  // the fragment row this lane supplies (ds_read_b64_tr_b16: four rows x four channel quads per 16 lanes)
        const bool ok = k < KR;
        const int ai = ok ? k / NA : 0, bi = ok ? k - ai * NA : 0;
        const int r = ai / WIN, wy = ai - r * WIN, s3 = bi / WIN, dx = bi - s3 * WIN;
        const int R = ok ? ((wcj + dx) * 9 + 3 * r + s3) : 0;          // padding: any staged row, its weight is zero
        araddr[ks][h] = (unsigned)(wy * SLOT + R * 128 + (((((L & 3) >> 1) ^ tm_swz(R))) << 4) + (L & 1) * 8);
      }
    }
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
      const int piece = wave + NW * i;
      const int R = piece * 8 + (lane >> 3);
      const int chunk = (lane & 7) ^ tm_swz(R);
      const int pc = R / 9, t = R - pc * 9;
      const int col = wcb0 + pc;
      const bool ok = piece < PIECES && R < ROWS && col >= 0 && col < Wi;
      doff[i] = ok ? (unsigned)((((col * 9 + t) * N) * 2) + chunk * 16) : kTmOob;
    }
    __syncthreads();
  }

  __device__ __forceinline__ void set_image(const uint16_t* z, int b) {
    srd = make_srd(z + (int64_t)b * Hi * (row_bytes / 2), (unsigned)((int64_t)Hi * row_bytes));
  }
  // one window row: (PIECES - wave + NW - 1) / NW instructions in wave `wave`; pad: MAXP in every wave (the pieces a wave does not
  // have are all-out-of-range fetches)
  __device__ __forceinline__ void issue_row(int cc, int y, int wave, unsigned lds_dummy, bool pad) const {
    const int yc = y < 0 ? 0 : (y > Hi - 1 ? Hi - 1 : y);
    const int slot = (y + 1) % NSLOT;
    const unsigned soff = (unsigned)((int64_t)yc * row_bytes) + (unsigned)(cc * 128);
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
      if (wave + NW * i < PIECES) dma16_buf(doff[i], srd, soff, lds + slot * SLOT + (wave + NW * i) * 1024);
      else if (pad) dma16_buf(kTmOob, srd, 0u, lds_dummy);
    }
  }
  // the window rows step s adds (step 0: the whole window, never padded).  A step s > 0 issues, with pad, NDMA = RPS rows x MAXP
  // instructions in every wave and step -- what a counted wait may rely on; without, the count differs between the waves (RPS x
  // the wave's pieces of a row) and, for factor 8, between the steps
  __device__ __forceinline__ void issue_step(int cc, int s, int wave, unsigned lds_dummy, bool pad) const {
    if (s == 0) {
#pragma unroll
      for (int y = 0; y < WIN; ++y) issue_row(cc, y - 1, wave, lds_dummy, false);
    } else if (LF == 1) {
      static_assert(LF != 1 || RPS == 2, "factor 2: two new rows per step");
      issue_row(cc, 2 * s + 1, wave, lds_dummy, pad);
      issue_row(cc, 2 * s + 2, wave, lds_dummy, pad);
    } else if (LF == 2) {
      static_assert(LF != 2 || RPS == 1, "factor 4: one new row per step");
      issue_row(cc, s + 1, wave, lds_dummy, pad);
    } else {                                               // factor 8: a new row every other step, one row's worth of padding in between
      if ((s & 1) == 0) issue_row(cc, (s >> 1) + 1, wave, lds_dummy, pad);
      else if (pad) {
#pragma unroll
        for (int i = 0; i < RPS * MAXP; ++i) dma16_buf(kTmOob, srd, 0u, lds_dummy);
      }
    }
  }
  // step i of the walk: acc += this source's share, for the NTN channel tiles nt0 .. of the wave's patch.  FIRST: the accumulators
  // are not initialised yet and start from addv.  ring = generic pointer to the ring.  PD = K-steps the fragment reads run ahead
  // of the matrix cores.
  template <bool FIRST, int PD, int NTN>
  __device__ __forceinline__ void compute(const unsigned char* ring, int i, bool top, bool bot, int nt0, f32x4_t (&acc)[NTN],
                                          const f32x4_t (&addv)[NTN]) const {
    const int cell0 = LF == 1 ? 2 * i : (LF == 2 ? i : (i >> 1));
    unsigned s0b = (unsigned)((cell0 % NSLOT) * SLOT);     // byte offset of the slot of the step's first window row
    asm volatile("" : "+s"(s0b));                          // (opaque: no unrolling over the ring's period with every address kept)
    auto run = [&](auto which, auto phase) {
      constexpr int PH = decltype(phase)::value, WH = decltype(which)::value;   // WH: 0 interior, 1 first step, 2 last step
      tm_s16x8_t zb[PD + 1][NTN];
      auto load = [&](int ks, tm_s16x8_t (&zf)[NTN]) {
        unsigned ad[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const unsigned v = araddr[ks][h] + s0b;          // (window row + first slot) mod NSLOT: the offset stays below 2 BYTES
          const unsigned t = v - (unsigned)BYTES;
          ad[h] = v < t ? v : t;                           // unsigned min: t wrapped around when v < BYTES
        }
#pragma unroll
        for (int j = 0; j < NTN; ++j) {
          const unsigned xm = (unsigned)((nt0 + j) << 5);
          const tm_s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tm_lds_s16x4_ptr)(ring + (ad[0] ^ xm)));
          const tm_s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tm_lds_s16x4_ptr)(ring + (ad[1] ^ xm)));
          zf[j] = tm_s16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
      };
#pragma unroll
      for (int ks = 0; ks < PD; ++ks)
        if (ks < NKS) load(ks, zb[ks % (PD + 1)]);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        if (ks + PD < NKS) load(ks + PD, zb[(ks + PD) % (PD + 1)]);
        bf16x8_t w = wf[PH][ks];
        if constexpr (WH != 0) {                           // the zero padding: two steps of a column pay ~25 instructions per K-step here
          const unsigned bits = ((WH == 1 ? mtop[ks >> 2] : mbot[ks >> 2]) >> (8 * (ks & 3))) & 0xffu;
          const uint4 wz = __builtin_bit_cast(uint4, w);
          unsigned wr[4] = {wz.x, wz.y, wz.z, wz.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const unsigned m2 = (bits >> (2 * q)) & 3u;
            wr[q] &= ~(((m2 & 1u) * 0xffffu) | ((m2 >> 1) * 0xffff0000u));
          }
          w = __builtin_bit_cast(bf16x8_t, make_uint4(wr[0], wr[1], wr[2], wr[3]));
        }
#pragma unroll
        for (int j = 0; j < NTN; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, zb[ks % (PD + 1)][j]), w, (FIRST && ks == 0) ? addv[j] : acc[j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // (the walk has at least two steps: the first one is never the last)
    if (top) run(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
    else if (bot) run(std::integral_constant<int, 2>{}, std::integral_constant<int, NPH - 1>{});
    else if (NPH == 2 && (i & 1)) run(std::integral_constant<int, 0>{}, std::integral_constant<int, NPH - 1>{});
    else run(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
  }
};

struct TapRArgs {
  const uint16_t* z;
  uint16_t* out;
  const float* addvec;
  float* stats;
  int Hi, Wi, N, Ho, Wo, B, relu;
  int nstrips, G, ncols, nchunks;   // strips per image row, column groups per XCD, columns = B * chunks, chunks = N / 64
};

// accumulators of a step -> (ReLU) -> bf16 -> the LDS tile [4 rows][16 pixels] x 128 B, 16-byte slots swizzled by pixel
template <int NTN>
__device__ __forceinline__ void roll_to_tile(unsigned char* tile, const f32x4_t (&acc)[NTN], int relu, int oxb0, int Wo, int lane, int pw, int nt0) {
  int t = lane;
  asm volatile("" : "+v"(t));
  const int l = t & 15, gq = t >> 4;
  const int pp = (l >> 2) * 16 + 4 * pw + (l & 3);
  const bool pxvalid = oxb0 + 4 * pw + (l & 3) < Wo;
#pragma unroll
  for (int j = 0; j < NTN; ++j) {
    const int ch = 16 * (nt0 + j) + 4 * gq;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = acc[j][e];
      if (relu) v[e] = fmaxf(v[e], 0.f);
      v[e] = pxvalid ? v[e] : 0.f;                         // columns beyond the image: zeros (not stored; the statistics count them as nothing)
    }
    *(uint2*)(tile + pp * 128 + ((((ch >> 3) ^ (pp & 7))) << 4) + (ch & 7) * 2) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
  }
}

template <int LF, bool STATS, int D>
__global__ __launch_bounds__(kRollThreads, LF == 2 ? 3 : 2) void resize_conv3x3_fwd_sum_roll_kernel(const TapRArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using S = RollSrc<LF, D>;                                // dynamic LDS = kTapTileBytes + S::BYTES (the launcher reads it off the same type)
  constexpr int STORES = tap_stores_per_flush(kTapTileBytes, kRollThreads);   // output stores per thread and flush
  static_assert(kRollThreads == 64 * S::NWAVES, "one-source kernel: the ring's pieces are dealt to the workgroup's waves");
  static_assert(STORES * kRollThreads * 16 == kTapTileBytes, "one-source kernel: the tile is exactly threads * stores * 16 bytes");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = lane & 15, g = lane >> 4;
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int grp = idx / a.nstrips, strip = idx - grp * a.nstrips;
  const int oxb0 = strip * 16;
  unsigned char* tile = smem;                              // [4 rows][16 pixels] x 128 B; the two weight tables during the set-up
  const unsigned char* ring = smem + kTapTileBytes;
  S s;
  s.setup((float*)tile, (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) void*)(smem + kTapTileBytes)),
          a.Hi, a.Wi, a.Wo, a.N, oxb0, tid, wave);
  const int nsteps = a.Ho >> 2;
  const bool fullstrip = oxb0 + 16 <= a.Wo;                // every thread stores its STORES pieces of every tile
  const int npw = (S::PIECES - wave + S::NWAVES - 1) / S::NWAVES;   // DMA instructions of this wave per window row (issue_row, not padded)
  const int gg = xcd * a.G + grp, gstride = 8 * a.G;
  bool primed = false;
  for (int col = gg; col < a.ncols; col += gstride) {
    const int b = col / a.nchunks, c = col - b * a.nchunks;
    if (!primed) {
      s.set_image(a.z, b);
#pragma unroll
      for (int q = 0; q < D; ++q)
        if (q < nsteps) s.issue_step(c, q, wave, 0u, false);
    }
    // the accumulators start from the per-channel addend (kept in registers for the column: no ordinary load -- whose wait the
    // compiler would place without knowing of the fetches in flight -- inside the step loop)
    f32x4_t addv[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const float4 v = a.addvec ? *(const float4*)(a.addvec + c * 64 + 16 * nt + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
      addv[nt] = f32x4_t{v.x, v.y, v.z, v.w};
    }
    f32x4_t sd1 = {0.f, 0.f, 0.f, 0.f}, sd2 = {0.f, 0.f, 0.f, 0.f};
    uint16_t* obase = a.out + (int64_t)b * a.Ho * a.Wo * a.N + c * 64;
    auto flush = [&](int step) {                           // the tile of `step` -> global memory (+ statistics)
      int t = tid;
      asm volatile("" : "+v"(t));                          // (addresses from an opaque thread id: not kept in registers across the steps)
      uint16_t* orow = obase + (int64_t)step * 4 * a.Wo * a.N;
#pragma unroll
      for (int u = 0; u < STORES; ++u) {
        const int i = t + kRollThreads * u, pp = i >> 3, chunk = i & 7;
        const uint4 v = *(const uint4*)(tile + pp * 128 + ((chunk ^ (pp & 7)) << 4));
        if (oxb0 + (pp & 15) < a.Wo) *(uint4*)(orow + ((int64_t)(pp >> 4) * a.Wo + oxb0 + (pp & 15)) * a.N + chunk * 8) = v;
      }
      if constexpr (STATS) {                               // wave w: channels 16 w .. 16 w + 15 of the chunk, all 64 pixels
        const int l = t & 15, gq = (t >> 4) & 3;
        const tm_s16x8_t one8 = {0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80};
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          const int p0 = 32 * k2 + 8 * gq + (l >> 2), p1 = p0 + 4;
          const int base = (l & 1) * 8, s16 = 2 * wave + ((l & 3) >> 1);
          const tm_s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tm_lds_s16x4_ptr)(tile + p0 * 128 + ((s16 ^ (p0 & 7)) << 4) + base));
          const tm_s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tm_lds_s16x4_ptr)(tile + p1 * 128 + ((s16 ^ (p1 & 7)) << 4) + base));
          const tm_s16x8_t zv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          const bf16x8_t f = __builtin_bit_cast(bf16x8_t, zv);
          sd1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, one8), f, sd1, 0, 0, 0);
          sd2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f, f, sd2, 0, 0, 0);
        }
      }
    };
#pragma unroll 1
    for (int i = 0; i < nsteps; ++i) {
      // (lgkmcnt(0) in every wait: hipcc drops its own LDS wait in front of the barrier below -- behind these asm statements the
      // last ds_write of the previous step's tile was still in flight when other waves read the tile: one patch row of the last
      // channel tile wrong in 1 of 4 launches)
      // this wave's pieces of step i's rows have landed.  Steady state (the fetch of step i was followed by STORES stores, then
      // D - 1 times by a fetch of S::RPS rows and STORES stores): those may stay in flight.  A wave has S::MAXP pieces of a row or
      // one fewer (S::PIECES dealt to S::NWAVES waves); the immediate is a constant, hence one arm per count
      if (D > 1 && fullstrip && i > D && i + D <= nsteps) {
        if (npw == S::MAXP) wait_vmcnt_lgkm0<steady_vmcnt(D, S::RPS * S::MAXP, STORES)>();
        else if (npw == S::MAXP - 1) wait_vmcnt_lgkm0<steady_vmcnt(D, S::RPS * (S::MAXP - 1), STORES)>();
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      }
      __syncthreads();                                    // ... everyone's; step i - 1 is computed and its tile written
      if (i + D < nsteps) s.issue_step(c, i + D, wave, 0u, false);
      if (i > 0) flush(i - 1);
      f32x4_t acc[4];
      s.template compute<true, 1, 4>(ring, i, i == 0, i == nsteps - 1, 0, acc, addv);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __syncthreads();                                    // everyone has flushed the previous tile
      roll_to_tile<4>(tile, acc, a.relu, oxb0, a.Wo, lane, wave, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();                                      // the last tile is written; nobody reads the ring any more
    const int ncol = col + gstride;
    primed = ncol < a.ncols;
    if (primed) {                                          // the next column's first rows travel under this column's tail
      const int nb = ncol / a.nchunks, nc = ncol - nb * a.nchunks;
      s.set_image(a.z, nb);
#pragma unroll
      for (int q = 0; q < D; ++q)
        if (q < nsteps) s.issue_step(nc, q, wave, 0u, false);
    }
    flush(nsteps - 1);
    if constexpr (STATS) {
      const int64_t prow = (int64_t)b * a.nstrips + strip;
      float* srow = a.stats + prow * 2 * a.N + c * 64 + 16 * wave + L;
      if (g == 0) srow[0] = sd1[0];
      if (g == (L >> 2)) {
        const int e = L & 3;
        srow[a.N] = e == 0 ? sd2[0] : (e == 1 ? sd2[1] : (e == 2 ? sd2[2] : sd2[3]));
      }
    }
  }
}

struct TapR3Args {
  const uint16_t* z[3];
  int H[3], W[3];
  uint16_t* out;
  const float* addvec;
  int N, Ho, Wo, B, relu;
  int nstrips, nstreams, ncols, nchunks, nblocks;
  int dbg;                          // tuning probes (gdl_debug_set_tapsum_roll >= 16): 16 = no matrix-core work, 32 = no row fetches after the first window, 64 = no stores
};

// 512 threads: wave w works on patch w & 3 and the channel tiles 2 (w >> 2), 2 (w >> 2) + 1 -- two waves per SIMD, so that one's LDS
// round trips and address arithmetic run under the other's matrix-core work (with 256 threads the waves were issuing 60 % of
// their cycles and parked the rest: 720 us of compute against 608 us for all memory traffic)
// the three rings and the LDS layout of the kernel below (the launcher's dynamic LDS size is BYTES of the same type)
template <int D>
struct Roll3Lds {
  static constexpr int NW = kRoll3Threads / 64;
  using SA = RollSrc<1, D, NW>;
  using SB = RollSrc<2, D, NW>;
  using SC = RollSrc<3, D, NW>;
  static constexpr int OA = kTapTileBytes, OB = OA + SA::BYTES, OC = OB + SB::BYTES, OD = OC + SC::BYTES;   // rings and the spare KiB behind the tile
  static constexpr int BYTES = OD + 1024;
  static_assert(BYTES <= 160 * 1024, "LDS budget");
};

template <int D>
__global__ __launch_bounds__(kRoll3Threads, 1) void resize_conv3x3_fwd_sum_roll3_kernel(const TapR3Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Lds = Roll3Lds<D>;
  using SA = typename Lds::SA;
  using SB = typename Lds::SB;
  using SC = typename Lds::SC;
  constexpr int NTN = 2;
  constexpr bool PAD = true;                               // what the three steady-state issue_step calls pass: the same count in every wave and step
  constexpr int NDMA = SA::NDMA + SB::NDMA + SC::NDMA;     // per wave and steady-state step
  static_assert(PAD, "roll3: every wave issues NDMA fetches per step (pad=true): the counted wait relies on it");
  constexpr int STORES = tap_stores_per_flush(kTapTileBytes, kRoll3Threads);   // output stores per thread and flush
  static_assert(STORES * kRoll3Threads * 16 == kTapTileBytes, "roll3: the tile is exactly threads * stores * 16 bytes");
  constexpr int OA = Lds::OA, OB = Lds::OB, OC = Lds::OC, OD = Lds::OD;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pw = wave & 3, nt0 = 2 * (wave >> 2);
  // workgroup -> (stream of columns, strip): the workgroups of one XCD take consecutive pairs, so the strips of a stream sit on one XCD
  // (a stream that straddles two XCDs fetches the two window columns at that seam twice)
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  int pair = idx;
  for (int x = 0; x < xcd; ++x) pair += (a.nblocks - x + 7) >> 3;
  const int stream = pair / a.nstrips, strip = pair - stream * a.nstrips;
  const int oxb0 = strip * 16;
  unsigned char* tile = smem;
  auto lds_of = [](unsigned char* p) { return (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) void*)p); };
  const unsigned lds_dummy = lds_of(smem + OD);
  SA sa; SB sb; SC sc;
  sa.setup((float*)tile, lds_of(smem + OA), a.H[0], a.W[0], a.Wo, a.N, oxb0, tid, wave);
  sb.setup((float*)tile, lds_of(smem + OB), a.H[1], a.W[1], a.Wo, a.N, oxb0, tid, wave);
  sc.setup((float*)tile, lds_of(smem + OC), a.H[2], a.W[2], a.Wo, a.N, oxb0, tid, wave);
  const int nsteps = a.Ho >> 2;
  const bool fullstrip = oxb0 + 16 <= a.Wo;
  const int g = lane >> 4;
  bool primed = false;
  for (int col = stream; col < a.ncols; col += a.nstreams) {
    const int b = col / a.nchunks, c = col - b * a.nchunks;
    if (!primed) {
      sa.set_image(a.z[0], b); sb.set_image(a.z[1], b); sc.set_image(a.z[2], b);
#pragma unroll
      for (int s = 0; s < D; ++s)
        if (s < nsteps) { sa.issue_step(c, s, wave, lds_dummy, false); sb.issue_step(c, s, wave, lds_dummy, false); sc.issue_step(c, s, wave, lds_dummy, false); }
    }
    f32x4_t addv[NTN];
#pragma unroll
    for (int j = 0; j < NTN; ++j) {
      const float4 v = a.addvec ? *(const float4*)(a.addvec + c * 64 + 16 * (nt0 + j) + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
      addv[j] = f32x4_t{v.x, v.y, v.z, v.w};
    }
    uint16_t* obase = a.out + (int64_t)b * a.Ho * a.Wo * a.N + c * 64;
    auto flush = [&](int step) {                           // 512 threads x 16 bytes = the tile
      static_assert(STORES == 1, "roll3: flush() issues one store per thread; more stores need a loop over STORES here");
      int t = tid;
      asm volatile("" : "+v"(t));
      uint16_t* orow = obase + (int64_t)step * 4 * a.Wo * a.N;
      const int pp = t >> 3, chunk = t & 7;
      const uint4 v = *(const uint4*)(tile + pp * 128 + ((chunk ^ (pp & 7)) << 4));
      if (oxb0 + (pp & 15) < a.Wo) *(uint4*)(orow + ((int64_t)(pp >> 4) * a.Wo + oxb0 + (pp & 15)) * a.N + chunk * 8) = v;
    };
#pragma unroll 1
    for (int i = 0; i < nsteps; ++i) {
      // (lgkmcnt(0) with every wait: see the one-source kernel.)  Steady state: the fetch of step i was followed by STORES stores,
      // then D - 1 times by a fetch (NDMA instructions in every wave) and STORES stores
      if (D > 1 && fullstrip && i > D && i + D <= nsteps) wait_vmcnt_lgkm0<steady_vmcnt(D, NDMA, STORES)>();
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __syncthreads();
      if (i + D < nsteps && !(a.dbg & 32)) {
        sa.issue_step(c, i + D, wave, lds_dummy, PAD); sb.issue_step(c, i + D, wave, lds_dummy, PAD); sc.issue_step(c, i + D, wave, lds_dummy, PAD);
      }
      if (i > 0 && !(a.dbg & 64)) flush(i - 1);
      f32x4_t acc[NTN];
      const bool top = i == 0, bot = i == nsteps - 1;
      if (a.dbg & 16) {
#pragma unroll
        for (int j = 0; j < NTN; ++j) acc[j] = addv[j];
      } else {
        sa.template compute<true, 1, NTN>(smem + OA, i, top, bot, nt0, acc, addv);
        sb.template compute<false, 1, NTN>(smem + OB, i, top, bot, nt0, acc, addv);
        sc.template compute<false, 1, NTN>(smem + OC, i, top, bot, nt0, acc, addv);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __syncthreads();
      roll_to_tile<NTN>(tile, acc, a.relu, oxb0, a.Wo, lane, pw, nt0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    const int ncol = col + a.nstreams;
    primed = ncol < a.ncols;
    if (primed) {
      const int nb = ncol / a.nchunks, nc = ncol - nb * a.nchunks;
      sa.set_image(a.z[0], nb); sb.set_image(a.z[1], nb); sc.set_image(a.z[2], nb);
#pragma unroll
      for (int s = 0; s < D; ++s)
        if (s < nsteps) { sa.issue_step(nc, s, wave, lds_dummy, false); sb.issue_step(nc, s, wave, lds_dummy, false); sc.issue_step(nc, s, wave, lds_dummy, false); }
    }
    flush(nsteps - 1);
  }
}

int g_tapsum_mfma = 1;     // A/B hook (gdl_debug_set_tapsum_mfma): 0 = the pixel-by-pixel kernel; 1 = MFMA, version chosen by shape;
                           // 5 = version 2 (4 x 16 pixel blocks, all channels, pipelined); 2 / 4 = version 1 (32- / 16-column blocks x 64 channels)
int g_tapsum_vec = 0;      // A/B hook (gdl_debug_set_tapsum_vec): 4 = 8-byte bf16 vectors per thread instead of 16-byte ones

}  // namespace

// ---- the same sum for ANY resize ratio (round 5): out[b, oy, ox, n] (+)= sum_(r,s) bilinear(z_(r,s))[oy + r - 1, ox + s - 1].
// The kernels above are built around an integer factor (a cell of F output columns shares its source columns); DOFA-large's
// top FPN level is int(73 * 0.5) = 36 pixels wide against 292 (models/utils.py:106-110: x 8.11), which sent the whole
// `fpn_bottleneck` to the unfused path (concat buffer + a K = 9 * 4096 convolution at full resolution).  This is the plain
// gather form -- per output vector 9 taps x 4 corners = 36 loads, f32 accumulation in a fixed order -- for the ONE level of a
// pyramid that needs it: the source is small (it is the level being upsampled ~8 x) and stays in L2.
template <typename V, int VEC>
__global__ __launch_bounds__(256) void resize_conv3x3_fwd_sum_any_kernel(const void* __restrict__ z, int Hi, int Wi, int N, void* out,
                                                                         int Ho, int Wo, int accumulate,
                                                                         const float* __restrict__ addvec, int relu) {
  const int cv = N / VEC;
  const int j0 = blockIdx.x * 256 + threadIdx.x;
  if (j0 >= Wo * cv) return;
  const int b = blockIdx.y / Ho, oy = blockIdx.y - b * Ho;
  const int ox = j0 / cv, c = (j0 - ox * cv) * VEC;
  const float ry = (float)Hi / (float)Ho, rx = (float)Wi / (float)Wo;
  const int64_t pix = 9ll * N;
  const int64_t zb = (int64_t)b * Hi * Wi * pix + c;
  float acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
  int xs0[3], xs1[3]; float lxs[3]; bool xin[3];
#pragma unroll
  for (int s3 = 0; s3 < 3; ++s3) {
    const int px = ox + s3 - 1;
    xin[s3] = px >= 0 && px < Wo;
    xs0[s3] = xs1[s3] = 0; lxs[s3] = 0.f;
    if (xin[s3]) src_index2(rx, px, Wi, xs0[s3], xs1[s3], lxs[s3]);
  }
#pragma unroll 1
  for (int r = 0; r < 3; ++r) {
    const int py = oy + r - 1;
    if (py < 0 || py >= Ho) continue;              // the convolution's zero padding (uniform over the block)
    int y0, y1; float ly;
    src_index2(ry, py, Hi, y0, y1, ly);
#pragma unroll
    for (int s3 = 0; s3 < 3; ++s3) {
      if (!xin[s3]) continue;
      const int64_t t = (int64_t)(3 * r + s3) * N;
      float v00[VEC], v01[VEC], v10[VEC], v11[VEC];
      V::ld(z, zb + ((int64_t)y0 * Wi + xs0[s3]) * pix + t, v00);
      V::ld(z, zb + ((int64_t)y0 * Wi + xs1[s3]) * pix + t, v01);
      V::ld(z, zb + ((int64_t)y1 * Wi + xs0[s3]) * pix + t, v10);
      V::ld(z, zb + ((int64_t)y1 * Wi + xs1[s3]) * pix + t, v11);
      const float lx = lxs[s3];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float top = v00[e] + lx * (v01[e] - v00[e]), bot = v10[e] + lx * (v11[e] - v10[e]);
        acc[e] += top + ly * (bot - top);
      }
    }
  }
  const int64_t o = (((int64_t)b * Ho + oy) * Wo + ox) * N + c;
  if (accumulate) {
    float prev[VEC];
    V::ld(out, o, prev);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] += prev[e];
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    if (addvec) acc[e] += addvec[c + e];
    if (relu) acc[e] = fmaxf(acc[e], 0.f);
  }
  V::st(out, o, acc);
}

extern "C" void gdl_debug_set_tapsum_vec(int vec) { g_tapsum_vec = vec; }
extern "C" void gdl_debug_set_tapsum_mfma(int mode) { g_tapsum_mfma = mode; }

static int g_tapsum_persist = 1;
extern "C" void gdl_debug_set_tapsum_persist(int on) { g_tapsum_persist = on; }  // A/B hook: 0 = one workgroup per patch (round 3)
static std::atomic<int> g_tapsum_cus{0};       // the device's CU count once a launch has asked for it
static int tapsum_num_cus() {      // (the plan query below must not enter the HIP runtime: it reads what a launch left here)
  const int cus = gdl_num_cus();
  g_tapsum_cus.store(cus);
  return cus;
}
static int g_tapsum_roll = 1;
constexpr int kRollDepth4 = 3;    // factor 4: steps the row fetches of version 3 run ahead (ring of RollSrc<2, depth>::NSLOT = 3 + depth slots, three workgroups per CU)
constexpr int kRoll3Depth = 2;    // the same for the three rings of roll3
extern "C" void gdl_debug_set_tapsum_roll(int on) { g_tapsum_roll = on; }  // A/B hook: 0 = versions 1 / 2 where version 3 (rolling row window) applies

// The form of the forward gather-sum for one call: what tapsum_launch runs and what gdl_resize_conv3x3_fwd_sum_plan reports.
// Every choice between kernels, template instantiations and grid shapes is made HERE (from the shape, the hooks and the CU
// count); the launcher only fills argument structs from it.
enum { TAP_VALU = 0, TAP_V1 = 1, TAP_V2 = 2, TAP_ROLL = 3, TAP_ROLL3 = 4 };
struct TapPlan {
  int kind;            // TAP_*
  int p, q;            // VALU: elements per vector (4 / 8), pixels per run (2 / 4 / 8); version 1: 16-column units per block (1 / 2), 0;
                       // version 2: NSRC, LF of the instantiation (0 for several sources); rolling window: LF, depth; roll3: 3, depth
  int walks;           // a workgroup takes more than one patch (version 2: the persistent grid) / column (rolling forms)
  int F[3], LF[3], run, lfmin;
  int nblk, grid;      // version 2: patches, workgroups launched; rolling window: columns, 8 * G * nstrips; roll3: columns, streams * nstrips
  int G;               // rolling window: column groups per XCD; roll3: streams
  int code() const { return 1000 * kind + 100 * p + 10 * q + walks; }
};
// out16 / add16: out / addvec are 16-byte aligned (every kernel stores vectors; the matrix-core kernels load the addend as vectors)
static int tapsum_plan(const int* hs, const int* ws, int nsrc, int dtype, int B, int N, int Ho, int Wo, bool stats, bool out16, bool add16,
                       int cus, TapPlan& t) {
  GDL_CHECK_ARG(hs && ws && nsrc >= 1 && nsrc <= 3, "gdl_resize_conv3x3_fwd_sum: 1..3 sources");
  GDL_CHECK_ARG(dtype == GDL_F32 || dtype == GDL_BF16, "gdl_resize_conv3x3_fwd_sum: bad dtype");
  GDL_CHECK_ARG(B > 0 && Ho > 0 && Wo > 0 && N > 0, "gdl_resize_conv3x3_fwd_sum: bad sizes");
  t = TapPlan{};
  t.run = 2; t.lfmin = 3;
  bool img_ok = out16;
  for (int k = 0; k < nsrc; ++k) {
    GDL_CHECK_ARG(hs[k] > 0 && ws[k] > 0, "gdl_resize_conv3x3_fwd_sum: bad source %d", k);
    const int f = Ho / hs[k];
    GDL_CHECK_ARG((f == 2 || f == 4 || f == 8) && hs[k] * f == Ho && ws[k] * f == Wo,
                  "gdl_resize_conv3x3_fwd_sum: source %d: the resize factor must be 2, 4 or 8 in both directions", k);
    t.F[k] = f; t.LF[k] = f == 8 ? 3 : (f == 4 ? 2 : 1);
    t.run = f > t.run ? f : t.run;
    t.lfmin = t.LF[k] < t.lfmin ? t.LF[k] : t.lfmin;
    img_ok = img_ok && (int64_t)hs[k] * ws[k] * 9 * N * 2 < 0x7ffffff0ll;   // 32-bit buffer offsets per image
  }
  for (int k = nsrc; k < 3; ++k) t.LF[k] = 1;      // (unused sources: as factor 0 always was)
  GDL_CHECK_ARG(Wo % t.run == 0, "gdl_resize_conv3x3_fwd_sum: Wo must be a multiple of the largest factor");
  const bool mfma_ok = dtype == GDL_BF16 && N % 64 == 0 && img_ok && (int64_t)B * ((Ho + 3) / 4) <= 65535 && add16;
  GDL_CHECK_ARG(!stats || mfma_ok, "gdl_resize_conv3x3_fwd_sum_bn: needs bf16, N %% 64 == 0, 16-byte aligned output and per-channel "
                "addend (bias), sources below 2 GiB per image, B * ceil(Ho / 4) <= 65535");
  if (mfma_ok && (g_tapsum_mfma || stats)) {
    const int nstrips = (Wo + 15) / 16, ncols = B * (N / 64);
    // version 3 for the three upsampled levels of fpn_bottleneck: factors 2, 4, 8 in that order, whole cells of the coarsest one
    if (g_tapsum_roll && !stats && nsrc == 3 && t.LF[0] == 1 && t.LF[1] == 2 && t.LF[2] == 3 && Ho % 8 == 0 && g_tapsum_mfma == 1) {
      int streams = cus / nstrips;            // one workgroup per CU
      if (streams > ncols) streams = ncols;
      if (streams < 1) streams = 1;
      t.kind = TAP_ROLL3; t.p = 3; t.q = kRoll3Depth;
      t.nblk = ncols; t.G = streams; t.grid = streams * nstrips; t.walks = ncols > streams;
      return GDL_OK;
    }
    // version 3 (rolling row window): one source of factor 2 or 4 whose output rows come in whole patches
    if (g_tapsum_roll && nsrc == 1 && (t.LF[0] == 1 || t.LF[0] == 2) && Ho % 4 == 0 && Ho >= 8 && (g_tapsum_mfma == 1 || stats)) {
      const int occ = t.LF[0] == 2 ? 3 : 2, slots = cus / 8 * occ;         // resident workgroups per XCD (launch bounds)
      int G = slots / nstrips;
      if (G > (ncols + 7) / 8) G = (ncols + 7) / 8;
      if (G < 1) G = 1;
      t.kind = TAP_ROLL; t.p = t.LF[0]; t.q = t.LF[0] == 2 ? (g_tapsum_roll == 2 ? 1 : kRollDepth4) : 1;      // (roll hook 2, A/B: one step ahead)
      t.nblk = ncols; t.G = G; t.grid = 8 * G * nstrips; t.walks = ncols > 8 * G;
      return GDL_OK;
    }
    // version 2 (all channels of a 4 x 16 pixel block per workgroup, windows double-buffered) where three blocks fit a CU: ONE
    // source of factor 4 or 8 (measured on the neck's x4 level: 442 us against 768; with the 46 KiB windows of a factor-2
    // source, or three sources, one block per CU remains and version 1 is the faster one: 284 vs 315 us, 693 vs 1148 us);
    // always for the statistics variant
    const bool v2_pays = nsrc == 1 && t.lfmin >= 2;
    if ((g_tapsum_mfma == 1 && v2_pays) || g_tapsum_mfma == 5 || stats) {
      const int cols = 16;   // (4 x 32 blocks: the cached fragments of two patches per wave do not fit the register budget)
      size_t ring = 0;
      for (int j = 0; j < (nsrc == 1 ? 2 : nsrc); ++j) ring += tap_window_bytes(cols, t.LF[nsrc == 1 ? 0 : j]);
      const size_t lds = (size_t)nsrc * (256 + cols * 64) + tap_tile_bytes(cols) + ring;
      GDL_CHECK_ARG(lds <= 160 * 1024 || !stats, "gdl_resize_conv3x3_fwd_sum_bn: LDS budget exceeded");
      if (lds <= 160 * 1024) {        // (always, for 1..3 sources of factors 2 / 4 / 8; version 1 below would take over)
        const int resident = cus * (nsrc == 1 ? 3 : 1);       // workgroups a launch keeps resident (launch bounds)
        t.kind = TAP_V2; t.p = nsrc; t.q = nsrc == 1 ? t.LF[0] : 0;
        t.nblk = ((Wo + cols - 1) / cols) * B * ((Ho + 3) / 4);
        t.walks = g_tapsum_persist && t.nblk > resident;
        t.grid = t.walks ? resident : t.nblk;
        return GDL_OK;
      }
    }
    // version 1: one block = 4 rows x 16 or 32 columns x 64 channels; 32 columns when every window stays under 48 KiB
    t.kind = TAP_V1; t.p = (tap_window_bytes(32, t.lfmin) <= 48 * 1024 && g_tapsum_mfma != 4) ? 2 : 1;
    return GDL_OK;
  }
  t.kind = TAP_VALU; t.p = dtype == GDL_BF16 ? 8 : 4; t.q = t.run;
  // 16-byte vectors with 8-pixel runs need more than 256 registers: 8-byte vectors there (and wherever N % 8 != 0)
  if (dtype == GDL_BF16 && (g_tapsum_vec == 4 || N % 8 != 0 || (t.run == 8 && g_tapsum_vec != 8))) t.p = 4;
  GDL_CHECK_ARG(N % t.p == 0 && out16, "gdl_resize_conv3x3_fwd_sum: N must be a multiple of 4, out 16-byte aligned");
  GDL_CHECK_ARG((int64_t)B * Ho <= 65535, "gdl_resize_conv3x3_fwd_sum: B * Ho must fit one grid dimension");
  return GDL_OK;
}

// The form gdl_resize_conv3x3_fwd_sum (with_stats: gdl_resize_conv3x3_fwd_sum_bn) takes for this call, for 16-byte aligned
// pointers, under the current gdl_debug_set_tapsum_* hooks: see include/gdlhip.h for the code.  A pure host query: no launch, no
// call into the HIP runtime -- the CU count is the one the launcher has seen, 256 (the MI355X's) before its first launch.
extern "C" int gdl_resize_conv3x3_fwd_sum_plan(const int* hs, const int* ws, int nsrc, int dtype, int B, int N, int Ho, int Wo,
                                               int with_stats) {
  TapPlan t;
  const int cus = g_tapsum_cus.load();
  if (tapsum_plan(hs, ws, nsrc, dtype, B, N, Ho, Wo, with_stats != 0, true, true, cus > 0 ? cus : 256, t) != GDL_OK) return -1;
  return t.code();
}

// shared launcher; stats != nullptr: per-block partial sums of the outputs ([rows][2][N] f32, rows = gdl_resize_conv3x3_fwd_sum_bn_rows)
// stat_rows (with stats): the number of partial rows the launch wrote (<= gdl_resize_conv3x3_fwd_sum_bn_rows)
static int tapsum_launch(const void* const* zs, const int* hs, const int* ws, int nsrc, int dtype, int B, int N, void* out, int Ho, int Wo,
                         const float* addvec, int relu, float* stats, hipStream_t st, int64_t* stat_rows = nullptr) {
  GDL_CHECK_ARG(zs && out, "gdl_resize_conv3x3_fwd_sum: 1..3 sources");
  TapPlan t;
  const int status = tapsum_plan(hs, ws, nsrc, dtype, B, N, Ho, Wo, stats != nullptr, (uintptr_t)out % 16 == 0, (uintptr_t)addvec % 16 == 0,
                                 tapsum_num_cus(), t);
  if (status != GDL_OK) return status;
  for (int k = 0; k < nsrc; ++k)
    GDL_CHECK_ARG(zs[k] && (uintptr_t)zs[k] % 16 == 0, "gdl_resize_conv3x3_fwd_sum: bad source %d", k);
  if (t.kind != TAP_VALU) {
    TapMArgs m;
    for (int k = 0; k < 3; ++k) {
      m.z[k] = k < nsrc ? (const uint16_t*)zs[k] : nullptr; m.H[k] = k < nsrc ? hs[k] : 1; m.W[k] = k < nsrc ? ws[k] : 1;
      m.LF[k] = t.LF[k];
    }
    m.nsrc = nsrc; m.N = N; m.Ho = Ho; m.Wo = Wo; m.B = B; m.out = (uint16_t*)out; m.addvec = addvec; m.relu = relu;
    m.nslots = 0; m.slot_off[0] = m.slot_off[1] = m.slot_off[2] = 0;
    if (stat_rows) *stat_rows = (int64_t)B * ((Ho + 3) / 4) * ((Wo + 15) / 16);
    if (t.kind == TAP_ROLL3) {
      TapR3Args r;
      for (int k = 0; k < 3; ++k) { r.z[k] = m.z[k]; r.H[k] = m.H[k]; r.W[k] = m.W[k]; }
      r.out = m.out; r.addvec = addvec; r.N = N; r.Ho = Ho; r.Wo = Wo; r.B = B; r.relu = relu;
      r.nstrips = (Wo + 15) / 16; r.nchunks = N / 64; r.ncols = t.nblk;
      r.nstreams = t.G; r.nblocks = t.grid;
      r.dbg = g_tapsum_roll >= 16 ? g_tapsum_roll : 0;
      GDL_SET_MAX_LDS_ONCE((resize_conv3x3_fwd_sum_roll3_kernel<kRoll3Depth>), 160 * 1024);
      hipLaunchKernelGGL((resize_conv3x3_fwd_sum_roll3_kernel<kRoll3Depth>), dim3((unsigned)r.nblocks), dim3(kRoll3Threads),
                         (size_t)Roll3Lds<kRoll3Depth>::BYTES, st, r);
      GDL_CHECK_LAUNCH("gdl_resize_conv3x3_fwd_sum");
      return GDL_OK;
    }
    if (t.kind == TAP_ROLL) {
      TapRArgs r;
      r.z = m.z[0]; r.out = m.out; r.addvec = addvec; r.stats = stats;
      r.Hi = m.H[0]; r.Wi = m.W[0]; r.N = N; r.Ho = Ho; r.Wo = Wo; r.B = B; r.relu = relu;
      r.nstrips = (Wo + 15) / 16; r.nchunks = N / 64; r.ncols = t.nblk;
      r.G = t.G;
      const dim3 grid((unsigned)t.grid);
      // (the dynamic LDS -- the tile and the ring -- is read off the RollSrc the instantiation indexes by)
#define TAPR(LF_, ST_, D_) do { constexpr size_t lds = kTapTileBytes + RollSrc<LF_, D_>::BYTES;                                          \
    static_assert(lds <= 160 * 1024, "LDS budget");                                                                                      \
    GDL_SET_MAX_LDS_ONCE((resize_conv3x3_fwd_sum_roll_kernel<LF_, ST_, D_>), 160 * 1024);                                                \
    hipLaunchKernelGGL((resize_conv3x3_fwd_sum_roll_kernel<LF_, ST_, D_>), grid, dim3(kRollThreads), lds, st, r); } while (0)
      if (t.p == 2 && t.q == 1) { if (stats) TAPR(2, true, 1); else TAPR(2, false, 1); }      // (A/B: one step ahead)
      else if (t.p == 2) { if (stats) TAPR(2, true, kRollDepth4); else TAPR(2, false, kRollDepth4); }
      else { if (stats) TAPR(1, true, 1); else TAPR(1, false, 1); }
#undef TAPR
      if (stat_rows) *stat_rows = (int64_t)B * r.nstrips;
      GDL_CHECK_LAUNCH("gdl_resize_conv3x3_fwd_sum");
      return GDL_OK;
    }
    if (t.kind == TAP_V2) {
      const int cols = 16;
      int ring = 0;
      m.nslots = nsrc == 1 ? 2 : nsrc;
      for (int j = 0; j < m.nslots; ++j) { m.slot_off[j] = ring; ring += tap_window_bytes(cols, m.LF[nsrc == 1 ? 0 : j]); }
      const size_t lds = (size_t)nsrc * (256 + cols * 64) + tap_tile_bytes(cols) + ring;
      m.gx = (Wo + cols - 1) / cols;
      m.nblk = t.nblk;
      const dim3 grid((unsigned)t.grid);
#define TAPM2(PXB_, NSRC_, LF_) do { GDL_SET_MAX_LDS_ONCE((resize_conv3x3_fwd_sum_mfma2_kernel<PXB_, NSRC_, LF_>), 160 * 1024);                 \
    hipLaunchKernelGGL((resize_conv3x3_fwd_sum_mfma2_kernel<PXB_, NSRC_, LF_>), grid, dim3(kTapM2Threads), lds, st, m, stats); } while (0)
      if (t.p == 1 && t.q == 2) TAPM2(4, 1, 2); else if (t.p == 1 && t.q == 3) TAPM2(4, 1, 3); else if (t.p == 1) TAPM2(4, 1, 1);
      else if (t.p == 2) TAPM2(4, 2, 0); else TAPM2(4, 3, 0);
#undef TAPM2
      GDL_CHECK_LAUNCH("gdl_resize_conv3x3_fwd_sum");
      return GDL_OK;
    }
    // version 1: one block = 4 rows x 16 or 32 columns x 64 channels
    const int cols = 16 * t.p;
    const int tile_bytes = tap_tile_bytes(cols), window = tap_window_bytes(cols, t.lfmin);
    const size_t lds = 256 + cols * 64 + (size_t)(window > tile_bytes ? window : tile_bytes);
    const dim3 grid((unsigned)(((Wo + cols - 1) / cols) * (N / 64)), (unsigned)(B * ((Ho + 3) / 4)));
    if (t.p == 2) {
      GDL_SET_MAX_LDS_ONCE(resize_conv3x3_fwd_sum_mfma_kernel<8>, 160 * 1024);
      hipLaunchKernelGGL(resize_conv3x3_fwd_sum_mfma_kernel<8>, grid, dim3(256), lds, st, m);
    } else {
      GDL_SET_MAX_LDS_ONCE(resize_conv3x3_fwd_sum_mfma_kernel<4>, 160 * 1024);
      hipLaunchKernelGGL(resize_conv3x3_fwd_sum_mfma_kernel<4>, grid, dim3(256), lds, st, m);
    }
    GDL_CHECK_LAUNCH("gdl_resize_conv3x3_fwd_sum");
    return GDL_OK;
  }
  TapSrc s;
  for (int k = 0; k < 3; ++k) {
    s.p[k] = k < nsrc ? zs[k] : nullptr; s.H[k] = k < nsrc ? hs[k] : 1; s.W[k] = k < nsrc ? ws[k] : 1; s.F[k] = k < nsrc ? t.F[k] : 0;
  }
  const int vec = t.p, run = t.run;
  const dim3 grid((unsigned)(((Wo / run) * (N / vec) + 255) / 256), (unsigned)(B * Ho));
#define TAPSUM(V, VEC, RUN) hipLaunchKernelGGL((resize_conv3x3_fwd_sum_kernel<V, VEC, RUN>), grid, dim3(256), 0, st, s, nsrc, N, out, \
                                               Ho, Wo, addvec, relu)
#define TAPSUM_RUN(V, VEC) do { if (run == 8) TAPSUM(V, VEC, 8); else if (run == 4) TAPSUM(V, VEC, 4); else TAPSUM(V, VEC, 2); } while (0)
  if (dtype == GDL_F32) TAPSUM_RUN(V4<float>, 4);
  else if (vec == 8) TAPSUM_RUN(V8, 8);
  else TAPSUM_RUN(V4<uint16_t>, 4);
#undef TAPSUM_RUN
#undef TAPSUM
  GDL_CHECK_LAUNCH("gdl_resize_conv3x3_fwd_sum");
  return GDL_OK;
}

extern "C" int gdl_resize_conv3x3_fwd_sum_any(const void* z, int hs, int ws, int dtype, int B, int N, void* out, int Ho, int Wo,
                                              int accumulate, const float* addvec, int relu, gdl_stream_t stream) {
  GDL_CHECK_ARG(z && out && hs > 0 && ws > 0 && B > 0 && N > 0 && Ho > 0 && Wo > 0, "gdl_resize_conv3x3_fwd_sum_any: bad args");
  GDL_CHECK_ARG(dtype == GDL_F32 || dtype == GDL_BF16, "gdl_resize_conv3x3_fwd_sum_any: bad dtype");
  const int vec = dtype == GDL_BF16 ? 8 : 4;
  GDL_CHECK_ARG(N % vec == 0 && (uintptr_t)z % 16 == 0 && (uintptr_t)out % 16 == 0,
                "gdl_resize_conv3x3_fwd_sum_any: N must be a multiple of the 16-byte vector, pointers 16-byte aligned");
  GDL_CHECK_ARG((int64_t)B * Ho <= 65535, "gdl_resize_conv3x3_fwd_sum_any: B * Ho must fit one grid dimension");
  const dim3 grid((unsigned)(((int64_t)Wo * (N / vec) + 255) / 256), (unsigned)(B * Ho));
  if (dtype == GDL_BF16)
    hipLaunchKernelGGL((resize_conv3x3_fwd_sum_any_kernel<V8, 8>), grid, dim3(256), 0, (hipStream_t)stream, z, hs, ws, N, out, Ho, Wo,
                       accumulate, addvec, relu);
  else
    hipLaunchKernelGGL((resize_conv3x3_fwd_sum_any_kernel<V4<float>, 4>), grid, dim3(256), 0, (hipStream_t)stream, z, hs, ws, N, out, Ho,
                       Wo, accumulate, addvec, relu);
  GDL_CHECK_LAUNCH("gdl_resize_conv3x3_fwd_sum_any");
  return GDL_OK;
}

extern "C" int gdl_resize_conv3x3_fwd_sum(const void* const* zs, const int* hs, const int* ws, int nsrc, int dtype, int B, int N,
                                          void* out, int Ho, int Wo, const float* addvec, int relu, gdl_stream_t stream) {
  return tapsum_launch(zs, hs, ws, nsrc, dtype, B, N, out, Ho, Wo, addvec, relu, nullptr, (hipStream_t)stream);
}

extern "C" int64_t gdl_resize_conv3x3_fwd_sum_bn_rows(int B, int Ho, int Wo) {
  if (B <= 0 || Ho <= 0 || Wo <= 0) return 0;
  return (int64_t)B * ((Ho + 3) / 4) * ((Wo + 15) / 16);
}

extern "C" int gdl_resize_conv3x3_fwd_sum_bn(const void* const* zs, const int* hs, const int* ws, int nsrc, int dtype, int B, int N,
                                             void* out, int Ho, int Wo, const float* addvec, float* workspace, int64_t ws_bytes,
                                             float* mean, float* var, float* running_mean, float* running_var, float momentum,
                                             gdl_stream_t stream) {
  GDL_CHECK_ARG(workspace && mean && var, "gdl_resize_conv3x3_fwd_sum_bn: null pointer");
  const int64_t rows = gdl_resize_conv3x3_fwd_sum_bn_rows(B, Ho, Wo);
  GDL_CHECK_ARG(ws_bytes >= rows * 2 * N * (int64_t)sizeof(float), "gdl_resize_conv3x3_fwd_sum_bn: workspace too small");
  int64_t written = rows;
  const int st = tapsum_launch(zs, hs, ws, nsrc, dtype, B, N, out, Ho, Wo, addvec, 0, workspace, (hipStream_t)stream, &written);
  if (st != GDL_OK) return st;
  return gdl_bn_stats_finalize(workspace, (int)written, N, (int64_t)B * Ho * Wo, mean, var, running_mean, running_var, momentum, stream);
}
