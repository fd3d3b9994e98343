// Raster preparation (include/gdlhip_raster.h): a raster resampled onto another grid, and the per-band sums of the dataset
// statistics.  The rule of the resampling is stated at the head of that header; tests/_raster_oracle.py restates it in numpy.
//
//   gdl_raster_warp: raster_taps_kernel fills, per destination column and per destination row, the tap table of the axis (first
//     tap, tap count, the sample that contains the centre, the float64 weights and their sum), once for all bands; then
//     raster_warp_kernel, a thread per destination pixel, walks its rows x columns of taps and carries the two sums in float64:
//     num = sum w_y (sum w_x m v), den = sum w_y (sum w_x m), one division at the end.  The x table is stored tap-major
//     ([tap][column]) so that the 64 lanes of a wave, which are 64 neighbouring columns of one row, read neighbouring weights; the
//     y table is the same for the whole wave.  The source is read through the caches: neighbouring lanes read neighbouring or the
//     same samples.  Nearest needs no table (raster_nearest_kernel).
//   gdl_raster_stats: raster_stats_kernel keeps (count, sum, sum of squares) per thread in 64-bit integers (integer kinds) or
//     float64 (float32), reduces them over the block in a fixed order, and then either adds the three integers to the accumulator
//     with integer atomics or stores the three float64 as the block's partial, which raster_stats_final_kernel adds up in a
//     fixed order.
#include "raster_common.h"
#include "../../include/gdlhip_raster.h"

#include <math.h>
#include <type_traits>

namespace {

constexpr int TILE_X = 64, TILE_Y = 4;      // destination pixels per workgroup of the warp: a wave is 64 columns of one row
constexpr int MAX_GRID = 1 << 20;           // workgroups of a launch; every kernel here walks its work with a grid stride
constexpr int STATS_UNROLL = 8;             // independent loads in flight per thread of the statistics pass

// ------------------------------------------------------------------ tap tables
struct AxisTable {      // of one axis of a destination of n entries, tmax taps at most
  int32_t* start;       // [n] first tap
  int32_t* count;       // [n] taps
  int32_t* centre;      // [n] floor(c) where that is a source sample, otherwise -1
  double* wsum;         // [n] the sum of the weights
  double* w;            // [tmax][n]
};

__device__ __forceinline__ double kernel_weight(double t, int cubic) {
  t = fabs(t);
  if (!cubic) return t < 1.0 ? 1.0 - t : 0.0;
  if (t < 1.0) return (1.5 * t - 2.5) * t * t + 1.0;
  if (t < 2.0) return ((-0.5 * t + 2.5) * t - 4.0) * t + 2.0;
  return 0.0;
}

// c = (i + 0.5) * s + o in float64, a product and a sum rounded one after the other: what any float64 restatement computes
__device__ __forceinline__ double centre_of(int i, double s, double o) { return __dadd_rn(__dmul_rn((double)i + 0.5, s), o); }

// `support` = R * f and `f` come from the host, so that no product here can be fused into the sums that pick the taps
__global__ void __launch_bounds__(256) raster_taps_kernel(AxisTable t, int n, int tmax, int nsrc, double s, double o, double f,
                                                           double support, int cubic) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double c = centre_of((int)i, s, o);
    const double lo = fmin(fmax(floor(__dadd_rn(__dadd_rn(c, -support), 0.5)), 0.0), (double)nsrc);
    const double hi = fmin(fmax(floor(__dadd_rn(__dadd_rn(c, support), 0.5)), 0.0), (double)nsrc);
    const int k0 = (int)lo;
    int cnt = (int)hi - k0;
    cnt = cnt < 0 ? 0 : (cnt > tmax ? tmax : cnt);      // tmax >= the rule's count (raster_tmax): the clamp guards the table alone
    double sum = 0.0;
    for (int j = 0; j < cnt; ++j) {
      const double w = kernel_weight(((double)(k0 + j) + 0.5 - c) / f, cubic);
      t.w[(int64_t)j * n + i] = w;
      sum += w;
    }
    t.start[i] = k0;
    t.count[i] = cnt;
    t.centre[i] = c >= 0.0 && c < (double)nsrc ? (int)floor(c) : -1;
    t.wsum[i] = sum;
  }
}

// ------------------------------------------------------------------ the destination's value
template <typename D> struct DstRange;
template <> struct DstRange<uint8_t> { static constexpr double lo = 0.0, hi = 255.0; };
template <> struct DstRange<uint16_t> { static constexpr double lo = 0.0, hi = 65535.0; };
template <> struct DstRange<int16_t> { static constexpr double lo = -32768.0, hi = 32767.0; };

template <typename D> __host__ __device__ __forceinline__ D round_to(double q) {      // integer D: floor(q + 0.5), clamped
  return (D)fmin(fmax(floor(q + 0.5), DstRange<D>::lo), DstRange<D>::hi);
}
template <> __host__ __device__ __forceinline__ float round_to<float>(double q) { return (float)q; }

template <typename D> __device__ __forceinline__ D quotient(double num, double den) { return round_to<D>(num / den); }
template <> __device__ __forceinline__ float quotient<float>(double num, double den) { return (float)num / (float)den; }

// the (ty, tx) tile of the grid-stride walk -> this thread's destination pixel; false outside the destination
__device__ __forceinline__ bool tile_pixel(int64_t tile, int tiles_x, int Hd, int Wd, int& y, int& x) {
  y = (int)(tile / tiles_x) * TILE_Y + threadIdx.y;
  x = (int)(tile % tiles_x) * TILE_X + threadIdx.x;
  return y < Hd && x < Wd;
}

template <typename S, typename D>
__global__ void __launch_bounds__(TILE_X* TILE_Y) raster_warp_kernel(const S* __restrict__ src, int H, int W, int Hd, int Wd,
                                                                      AxisTable tx, AxisTable ty, NoData nd, D fill,
                                                                      D* __restrict__ dst, uint8_t* __restrict__ valid) {
  const int tiles_x = (Wd + TILE_X - 1) / TILE_X;
  const int64_t tiles = (int64_t)tiles_x * ((Hd + TILE_Y - 1) / TILE_Y);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int y, x;
    if (!tile_pixel(tile, tiles_x, Hd, Wd, y, x)) continue;
    const int cy = ty.centre[y], cx = tx.centre[x];
    bool ok = cy >= 0 && cx >= 0 && !nd.masks((double)src[(int64_t)cy * W + cx]);
    D out = fill;
    if (ok) {
      const int y0 = ty.start[y], ny = ty.count[y], x0 = tx.start[x], nx = tx.count[x];      // inside the source by the table's clamp
      double num = 0.0, den = 0.0;
      for (int j = 0; j < ny; ++j) {
        const S* __restrict__ row = src + (int64_t)(y0 + j) * W + x0;
        double rn = 0.0, rd = 0.0;
        for (int i = 0; i < nx; ++i) {
          const double v = (double)row[i];
          const bool m = nd.masks(v);
          const double w = m ? 0.0 : tx.w[(int64_t)i * Wd + x];
          rn += w * (m ? 0.0 : v);      // a masked NaN must not reach the sum
          rd += w;
        }
        const double wy = ty.w[(int64_t)j * Hd + y];
        num += wy * rn;
        den += wy * rd;
      }
      ok = den >= GDL_RASTER_MIN_VALID_WEIGHT * (ty.wsum[y] * tx.wsum[x]);
      if (ok) out = quotient<D>(num, den);
    }
    const int64_t at = (int64_t)y * Wd + x;
    dst[at] = out;
    if (valid) valid[at] = ok;
  }
}

template <typename S, typename D>
__global__ void __launch_bounds__(TILE_X* TILE_Y) raster_nearest_kernel(const S* __restrict__ src, int H, int W, int Hd, int Wd,
                                                                         double sx, double ox, double sy, double oy, NoData nd,
                                                                         D fill, D* __restrict__ dst, uint8_t* __restrict__ valid) {
  const int tiles_x = (Wd + TILE_X - 1) / TILE_X;
  const int64_t tiles = (int64_t)tiles_x * ((Hd + TILE_Y - 1) / TILE_Y);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int y, x;
    if (!tile_pixel(tile, tiles_x, Hd, Wd, y, x)) continue;
    const double u = centre_of(x, sx, ox), v = centre_of(y, sy, oy);
    bool ok = u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H;
    D out = fill;
    if (ok) {
      const S s = src[(int64_t)floor(v) * W + (int64_t)floor(u)];
      ok = !nd.masks((double)s);
      if (ok) out = (D)s;
    }
    const int64_t at = (int64_t)y * Wd + x;
    dst[at] = out;
    if (valid) valid[at] = ok;
  }
}

// ------------------------------------------------------------------ statistics
template <typename A> __device__ __forceinline__ A wave_total(A v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the block's total in thread 0: the waves' totals (a fixed tree) added in the order of the waves
template <typename A> __device__ __forceinline__ A block_total(A v, A* lds) {
  v = wave_total(v);
  __syncthreads();      // lds may still be read from the total before
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

// A: int64_t for the integer kinds (acc += with integer atomics), double for float (partials[block] = the block's sums)
template <typename S, typename A>
__global__ void __launch_bounds__(256) raster_stats_kernel(const S* __restrict__ src, int64_t HW, NoData nd, int64_t* acc,
                                                            double* partials) {
  __shared__ A lds[4];
  const int64_t stride = (int64_t)gridDim.x * 256;
  A n = 0, s = 0, ss = 0;
  for (int64_t base = (int64_t)blockIdx.x * 256 + threadIdx.x; base < HW; base += stride * STATS_UNROLL) {
    S v[STATS_UNROLL];
#pragma unroll
    for (int u = 0; u < STATS_UNROLL; ++u) {
      const int64_t i = base + u * stride;
      v[u] = i < HW ? src[i] : S(0);
    }
#pragma unroll
    for (int u = 0; u < STATS_UNROLL; ++u) {
      const bool live = base + u * stride < HW && !nd.masks((double)v[u]);
      const A a = live ? (A)v[u] : A(0);
      n += live ? A(1) : A(0);
      s += a;
      ss += a * a;
    }
  }
  n = block_total(n, lds);
  s = block_total(s, lds);
  ss = block_total(ss, lds);
  if (threadIdx.x != 0) return;
  if constexpr (std::is_same<A, int64_t>::value) {
    atomicAdd((unsigned long long*)acc + 0, (unsigned long long)n);
    atomicAdd((unsigned long long*)acc + 1, (unsigned long long)s);
    atomicAdd((unsigned long long*)acc + 2, (unsigned long long)ss);
  } else {
    double* p = partials + (int64_t)blockIdx.x * 3;
    p[0] = n, p[1] = s, p[2] = ss;
  }
}

// one wave per band: lane l adds the partials l, l + 64, ... in that order, the lanes' sums go through a fixed tree
__global__ void __launch_bounds__(64) raster_stats_final_kernel(const double* __restrict__ partials, int blocks, int64_t* acc) {
  const double* p = partials + (int64_t)blockIdx.x * blocks * 3;
  double t[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < blocks; b += 64)
    for (int k = 0; k < 3; ++k) t[k] += p[(int64_t)b * 3 + k];
  for (int k = 0; k < 3; ++k) t[k] = wave_total(t[k]);
  if (threadIdx.x != 0) return;
  int64_t* a = acc + (int64_t)blockIdx.x * 3;
  a[0] += (int64_t)t[0];      // a count below 2^31 per call: exact in float64
  ((double*)a)[1] += t[1];
  ((double*)a)[2] += t[2];
}

// ------------------------------------------------------------------ host
// the taps of one axis at most: floor(c + R f + 0.5) - floor(c - R f + 0.5) <= ceil(2 R f)
inline int raster_tmax(double s, int method) { return (int)ceil(2.0 * method * fmax(1.0, s)) + 1; }

int check_geometry(const char* fn, int Hd, int Wd, double sx, double sy, int method) {
  GDL_CHECK_ARG(method >= GDL_RASTER_NEAREST && method <= GDL_RASTER_CUBIC, "%s: method %d is none of nearest (0), bilinear (1), cubic (2)", fn, method);
  GDL_CHECK_ARG(Hd > 0 && Wd > 0 && (int64_t)Hd * Wd < PIXEL_LIMIT, "%s: destination %d x %d: sizes must be positive and Hd * Wd < 2^31", fn, Hd, Wd);
  GDL_CHECK_ARG(sx > 0.0 && sy > 0.0 && isfinite(sx) && isfinite(sy), "%s: the scales must be positive and finite, got sx %g, sy %g", fn, sx, sy);
  GDL_CHECK_ARG(method == GDL_RASTER_NEAREST || (sx <= GDL_RASTER_MAX_SCALE && sy <= GDL_RASTER_MAX_SCALE),
                "%s: scale %g x %g: bilinear and cubic take a scale of at most %d (their support grows with it)", fn, sx, sy, GDL_RASTER_MAX_SCALE);
  return GDL_OK;
}

// the doubles of one axis' table, then its ints, carved out of ws; returns the first byte after them
struct TableLayout {
  static int64_t doubles(int n, int tmax) { return (int64_t)n * (tmax + 1); }
  static AxisTable carve(double*& d, int32_t*& i, int n, int tmax) {
    AxisTable t;
    t.wsum = d, t.w = d + n, d += doubles(n, tmax);
    t.start = i, t.count = i + n, t.centre = i + 2 * (int64_t)n, i += 3 * (int64_t)n;
    return t;
  }
};

inline dim3 tile_grid(int Hd, int Wd) {
  const int64_t tiles = (int64_t)((Wd + TILE_X - 1) / TILE_X) * ((Hd + TILE_Y - 1) / TILE_Y);
  return dim3((unsigned)(tiles < MAX_GRID ? tiles : MAX_GRID));
}

}  // namespace

extern "C" int64_t gdl_raster_warp_workspace(int Hd, int Wd, double sx, double sy, int method) {
  if (check_geometry("gdl_raster_warp_workspace", Hd, Wd, sx, sy, method)) return -1;
  if (method == GDL_RASTER_NEAREST) return 0;
  const int64_t doubles = TableLayout::doubles(Wd, raster_tmax(sx, method)) + TableLayout::doubles(Hd, raster_tmax(sy, method));
  return doubles * (int64_t)sizeof(double) + 3 * ((int64_t)Wd + Hd) * (int64_t)sizeof(int32_t);
}

extern "C" int gdl_raster_warp(const void* src, int kind, int C, int H, int W, int Hd, int Wd, double sx, double ox, double sy,
                               double oy, int method, const double* nodata, const uint8_t* has_nodata, double dst_nodata, void* dst,
                               int dst_kind, uint8_t* valid, void* ws, gdl_stream_t stream) {
  const char* fn = "gdl_raster_warp";
  if (const int bad = check_source(fn, kind, C, H, W)) return bad;
  if (const int bad = check_geometry(fn, Hd, Wd, sx, sy, method)) return bad;
  GDL_CHECK_ARG(isfinite(ox) && isfinite(oy), "%s: the offsets must be finite, got ox %g, oy %g", fn, ox, oy);
  GDL_CHECK_ARG(dst_kind == kind || dst_kind == GDL_RAW_F32, "%s: the destination is of the source's kind (%d) or float32, got kind %d", fn, kind, dst_kind);
  GDL_CHECK_ARG(src && dst, "%s: null pointer", fn);
  GDL_CHECK_ARG(method == GDL_RASTER_NEAREST || (ws && (uintptr_t)ws % 8 == 0), "%s: ws must be given and 8-byte aligned", fn);
  GDL_CHECK_ARG((uintptr_t)src % kind_size(kind) == 0 && (uintptr_t)dst % kind_size(dst_kind) == 0, "%s: src and dst must be aligned to their samples", fn);
  hipStream_t s = (hipStream_t)stream;

  AxisTable tx{}, ty{};
  if (method != GDL_RASTER_NEAREST) {
    const int tmx = raster_tmax(sx, method), tmy = raster_tmax(sy, method);
    double* d = (double*)ws;
    int32_t* i = (int32_t*)(d + TableLayout::doubles(Wd, tmx) + TableLayout::doubles(Hd, tmy));
    tx = TableLayout::carve(d, i, Wd, tmx);
    ty = TableLayout::carve(d, i, Hd, tmy);
    const double fx = fmax(1.0, sx), fy = fmax(1.0, sy), R = method;      // R = 1 bilinear, 2 cubic
    const int cubic = method == GDL_RASTER_CUBIC;
    hipLaunchKernelGGL(raster_taps_kernel, dim3(grid_for(Wd)), dim3(256), 0, s, tx, Wd, tmx, W, sx, ox, fx, R * fx, cubic);
    hipLaunchKernelGGL(raster_taps_kernel, dim3(grid_for(Hd)), dim3(256), 0, s, ty, Hd, tmy, H, sy, oy, fy, R * fy, cubic);
    GDL_CHECK_LAUNCH(fn);
  }

  const int64_t HW = (int64_t)H * W, HWd = (int64_t)Hd * Wd;
  const dim3 grid = tile_grid(Hd, Wd), block(TILE_X, TILE_Y);
  for (int c = 0; c < C; ++c) {
    const NoData nd = band_nodata(nodata, has_nodata, c);
    uint8_t* vp = valid ? valid + c * HWd : nullptr;
#define WARP(S, D)                                                                                                                     \
  if (method == GDL_RASTER_NEAREST)                                                                                                    \
    hipLaunchKernelGGL((raster_nearest_kernel<S, D>), grid, block, 0, s, (const S*)src + c * HW, H, W, Hd, Wd, sx, ox, sy, oy, nd,    \
                       round_to<D>(dst_nodata), (D*)dst + c * HWd, vp);                                                                \
  else                                                                                                                                 \
    hipLaunchKernelGGL((raster_warp_kernel<S, D>), grid, block, 0, s, (const S*)src + c * HW, H, W, Hd, Wd, tx, ty, nd,                \
                       round_to<D>(dst_nodata), (D*)dst + c * HWd, vp);
#define WARP_KIND(S)                          \
  if (dst_kind == kind) { WARP(S, S) }        \
  else { WARP(S, float) }
    if (kind == GDL_RAW_U8) { WARP_KIND(uint8_t) }
    else if (kind == GDL_RAW_U16) { WARP_KIND(uint16_t) }
    else if (kind == GDL_RAW_I16) { WARP_KIND(int16_t) }
    else { WARP(float, float) }
#undef WARP_KIND
#undef WARP
  }
  GDL_CHECK_LAUNCH(fn);
  return GDL_OK;
}

static int stats_blocks(int64_t HW) {
  const int64_t b = (HW + 256 * STATS_UNROLL - 1) / (256 * STATS_UNROLL);
  return (int)(b < GDL_RASTER_STATS_BLOCKS ? b : GDL_RASTER_STATS_BLOCKS);
}

extern "C" int64_t gdl_raster_stats_workspace(int kind, int C, int H, int W) {
  if (check_source("gdl_raster_stats_workspace", kind, C, H, W)) return -1;
  return kind == GDL_RAW_F32 ? (int64_t)C * GDL_RASTER_STATS_BLOCKS * 3 * (int64_t)sizeof(double) : 0;
}

extern "C" int gdl_raster_stats(const void* src, int kind, int C, int H, int W, const double* nodata, const uint8_t* has_nodata,
                                int64_t* acc, void* ws, gdl_stream_t stream) {
  const char* fn = "gdl_raster_stats";
  if (const int bad = check_source(fn, kind, C, H, W)) return bad;
  GDL_CHECK_ARG(src && acc, "%s: null pointer", fn);
  GDL_CHECK_ARG((uintptr_t)src % kind_size(kind) == 0 && (uintptr_t)acc % 8 == 0, "%s: src must be aligned to its samples and acc to 8 bytes", fn);
  GDL_CHECK_ARG(kind != GDL_RAW_F32 || (ws && (uintptr_t)ws % 8 == 0), "%s: float32 needs ws, 8-byte aligned", fn);
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const int blocks = stats_blocks(HW);
  for (int c = 0; c < C; ++c) {
    const NoData nd = band_nodata(nodata, has_nodata, c);
    double* part = kind == GDL_RAW_F32 ? (double*)ws + (int64_t)c * blocks * 3 : nullptr;
#define STATS(S, A) hipLaunchKernelGGL((raster_stats_kernel<S, A>), dim3(blocks), dim3(256), 0, s, (const S*)src + c * HW, HW, nd, acc + 3 * c, part);
    if (kind == GDL_RAW_U8) { STATS(uint8_t, int64_t) }
    else if (kind == GDL_RAW_U16) { STATS(uint16_t, int64_t) }
    else if (kind == GDL_RAW_I16) { STATS(int16_t, int64_t) }
    else { STATS(float, double) }
#undef STATS
  }
  if (kind == GDL_RAW_F32) hipLaunchKernelGGL(raster_stats_final_kernel, dim3(C), dim3(64), 0, s, (const double*)ws, blocks, acc);
  GDL_CHECK_LAUNCH(fn);
  return GDL_OK;
}
