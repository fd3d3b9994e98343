// Raster radiometry (include/gdlhip_raster_tone.h): per-band histograms, quantiles read off them, and the linear stretch to
// uint8 / float32.  The rules are stated at the head of that header; tests/_tone_oracle.py restates them in numpy.
//
//   gdl_raster_hist: raster_hist_kernel, one launch per band.  The band is cut into runs of HIST_THREADS * ITERS 16-byte
//     vectors (at most HIST_RUN = 65535 samples with the few samples in front of and behind the aligned body, which the first
//     run takes); a workgroup counts a run in an LDS table of two 16-bit counters to a word (one ds_add_u32 of 1 << 16 * (bin &
//     1) per sample), then adds the non-zero halves to acc with 64-bit integer atomics and zeroes them.  A half holds at most
//     the samples of one run, so it never carries into its neighbour, whatever the values: a constant raster fills one half
//     with at most 65535.  The 16-bit kinds and float32 use one table of 65538 halves (128 KiB: one workgroup per CU); uint8
//     a table of 256 halves per wave (8 KiB), added up in the flush.
//   gdl_raster_hist_quantiles: raster_quantiles_kernel, one workgroup per band: every thread sums a run of neighbouring bins,
//     an int64 scan over the threads gives each its exclusive prefix, and the thread whose run holds rank r walks it.
//   gdl_raster_stretch: raster_stretch_kernel, one launch per band, 16 samples per thread: 16-byte loads, float64 arithmetic,
//     16-byte stores; the samples in front of the first index at which source, destination and validity plane are all 16-byte
//     aligned, and those behind the last whole 16, go one by one.
// Nothing here may be contracted into a fused multiply-add: the rules are float64 "as written".
#include "raster_common.h"
#include "../../include/gdlhip_raster_tone.h"

#include <float.h>
#include <math.h>
#include <string.h>
#include <type_traits>

#pragma clang fp contract(off)

namespace {

constexpr int HIST_THREADS = 1024;
constexpr int HIST_RUN = 65535;                                   // what a 16-bit half can hold
constexpr int HIST_WORDS = (GDL_RASTER_TONE_MAX_BINS + 2) / 2;    // bins, under and over, two to a word
constexpr int HIST_GRID = 256;                                    // workgroups of the large table: one per CU, each zeroes it once
constexpr int QUANT_THREADS = 1024;
constexpr int STRETCH_UNIT = 16;                                  // samples per thread and step of the stretch

struct FloatBins {      // of a float32 band
  double lo, hi, d, bins;      // d = hi - lo, in float64
};

// the bin of a sample, or -1 for one that is counted nowhere
template <typename S> __device__ __forceinline__ int bin_of(S s, const NoData& nd, const FloatBins& fb) {
  const double v = (double)s;
  if (nd.masks(v)) return -1;
  if constexpr (std::is_same<S, float>::value) {
    if (v != v) return -1;
    const int bins = (int)fb.bins;
    if (v < fb.lo) return bins;
    if (v > fb.hi) return bins + 1;
    const double b = floor((v - fb.lo) / fb.d * fb.bins);
    return b < fb.bins ? (int)b : bins - 1;
  } else if constexpr (std::is_same<S, int16_t>::value) {
    return (int)s + 32768;
  } else {
    return (int)s;
  }
}

// the 16-byte vectors a thread takes of one run: with the samples in front of and behind the body, at most HIST_RUN samples
template <typename S> constexpr int hist_iters() {
  return (HIST_RUN - 2 * (16 / (int)sizeof(S) - 1)) / (HIST_THREADS * (16 / (int)sizeof(S)));
}

// WORDS: the words of one table; COPIES: tables per workgroup, one per group of HIST_THREADS / COPIES threads
template <typename S, int WORDS, int COPIES>
__global__ void __launch_bounds__(HIST_THREADS) raster_hist_kernel(const S* __restrict__ src, int64_t HW, int head, NoData nd,
                                                                    FloatBins fb, int words_used, int64_t* acc) {
  constexpr int VEC = 16 / (int)sizeof(S);
  constexpr int ITERS = hist_iters<S>();
  static_assert(ITERS >= 1 && ITERS * HIST_THREADS * VEC + 2 * (VEC - 1) <= HIST_RUN, "a run must fit a 16-bit counter");
  __shared__ uint32_t table[WORDS * COPIES];
  uint32_t* mine = table + (threadIdx.x / (HIST_THREADS / COPIES)) * WORDS;
  for (int w = threadIdx.x; w < WORDS * COPIES; w += HIST_THREADS) table[w] = 0;
  __syncthreads();

  const S* body = src + head;
  const int64_t nvec = (HW - head) / VEC;
  const int tail = (int)(HW - head - nvec * VEC);
  const int64_t runs = nvec > 0 ? (nvec + HIST_THREADS * ITERS - 1) / (HIST_THREADS * ITERS) : 1;
  auto count = [&](S s) {
    const int b = bin_of<S>(s, nd, fb);
    if (b >= 0) atomicAdd(&mine[b >> 1], 1u << (16 * (b & 1)));
  };
  for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
    if (run == 0) {      // fewer than VEC samples each
      if ((int)threadIdx.x < head) count(src[threadIdx.x]);
      if ((int)threadIdx.x < tail) count(body[nvec * VEC + threadIdx.x]);
    }
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int64_t vec = (run * ITERS + it) * HIST_THREADS + threadIdx.x;
      if (vec < nvec) {
        const uint4 raw = *reinterpret_cast<const uint4*>(body + vec * VEC);
        S v[VEC];
        memcpy(v, &raw, 16);
#pragma unroll
        for (int k = 0; k < VEC; ++k) count(v[k]);
      }
    }
    __syncthreads();
    for (int w = threadIdx.x; w < words_used; w += HIST_THREADS) {
      unsigned long long even = 0, odd = 0;
#pragma unroll
      for (int c = 0; c < COPIES; ++c) {
        const uint32_t n = table[c * WORDS + w];
        if (n) table[c * WORDS + w] = 0;
        even += n & 0xffffu;
        odd += n >> 16;
      }
      if (even) atomicAdd((unsigned long long*)acc + 2 * w, even);
      if (odd) atomicAdd((unsigned long long*)acc + 2 * w + 1, odd);      // an odd bin count: the last half is never counted in
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ quantiles
struct Quantiles {
  double q[GDL_RASTER_TONE_MAX_Q];
};

__global__ void __launch_bounds__(QUANT_THREADS) raster_quantiles_kernel(const int64_t* __restrict__ n, int bins, Quantiles qs, int Q,
                                                                          double origin, double step, double* __restrict__ out) {
  __shared__ int64_t waves[QUANT_THREADS / 64];
  const int per = (bins + QUANT_THREADS - 1) / QUANT_THREADS;      // at most 64 neighbouring bins per thread
  const int b0 = min((int)threadIdx.x * per, bins), b1 = min(b0 + per, bins);
  int64_t own = 0;
  for (int b = b0; b < b1; ++b) own += n[b];
  int64_t incl = own;      // inclusive scan over the wave, then over the waves
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t up = __shfl_up((long long)incl, o, 64);
    if ((threadIdx.x & 63) >= (unsigned)o) incl += up;
  }
  if ((threadIdx.x & 63) == 63) waves[threadIdx.x >> 6] = incl;
  __syncthreads();
  int64_t before = 0, N = 0;
  for (int w = 0; w < QUANT_THREADS / 64; ++w) {
    if (w < (int)(threadIdx.x >> 6)) before += waves[w];
    N += waves[w];
  }
  const int64_t first = before + incl - own;      // the samples in the bins before b0
  if (N == 0) {
    if ((int)threadIdx.x < Q) out[threadIdx.x] = nan("");
    return;
  }
  for (int j = 0; j < Q; ++j) {
    const int64_t r = (int64_t)floor(qs.q[j] * (double)(N - 1));
    if (r < first || r >= first + own) continue;      // exactly one thread holds rank r
    int64_t cum = first;
    for (int b = b0; b < b1; ++b) {
      cum += n[b];
      if (cum > r) {
        out[j] = origin + (double)b * step;
        break;
      }
    }
  }
}

// ------------------------------------------------------------------ stretch
template <typename D> __device__ __forceinline__ D tone_value(double y);
template <> __device__ __forceinline__ uint8_t tone_value<uint8_t>(double y) { return (uint8_t)fmin(fmax(floor(y + 0.5), 0.0), 255.0); }
template <> __device__ __forceinline__ float tone_value<float>(double y) { return (float)y; }

template <typename S, typename D>
__global__ void __launch_bounds__(256) raster_stretch_kernel(const S* __restrict__ src, int64_t HW, int64_t head, NoData nd,
                                                              const double* __restrict__ bounds, double out_lo, double out_span,
                                                              D fill, D* __restrict__ dst, uint8_t* __restrict__ valid) {
  constexpr int U = STRETCH_UNIT;
  const double lo = bounds[0], hi = bounds[1], d = hi - lo;
  const bool dead = !(isfinite(lo) && isfinite(hi) && isfinite(d));
  auto one = [&](S s, D& o) -> uint8_t {
    const double v = (double)s;
    if (dead || v != v || nd.masks(v)) {
      o = fill;
      return 0;
    }
    const double t = hi <= lo ? (v > lo ? 1.0 : 0.0) : fmin(fmax((v - lo) / d, 0.0), 1.0);
    o = tone_value<D>(out_lo + t * out_span);
    return 1;
  };
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  const int64_t units = (HW - head) / U, rest = head + units * U;
  for (int64_t u = tid; u < units; u += stride) {
    const int64_t at = head + u * U;
    S in[U];
    D o[U];
    uint8_t ok[U];
    uint4 raw[sizeof(S)];
#pragma unroll
    for (int k = 0; k < (int)sizeof(S); ++k) raw[k] = reinterpret_cast<const uint4*>(src + at)[k];
    memcpy(in, raw, sizeof(in));
#pragma unroll
    for (int k = 0; k < U; ++k) ok[k] = one(in[k], o[k]);
    uint4 res[sizeof(D)];
    memcpy(res, o, sizeof(o));
#pragma unroll
    for (int k = 0; k < (int)sizeof(D); ++k) reinterpret_cast<uint4*>(dst + at)[k] = res[k];
    if (valid) {
      uint4 v;
      memcpy(&v, ok, 16);
      *reinterpret_cast<uint4*>(valid + at) = v;
    }
  }
  for (int64_t i = tid; i < head + (HW - rest); i += stride) {      // in front of and behind the aligned body
    const int64_t at = i < head ? i : rest + (i - head);
    D o;
    const uint8_t ok = one(src[at], o);
    dst[at] = o;
    if (valid) valid[at] = ok;
  }
}

// ------------------------------------------------------------------ host
inline int kind_bins(int kind) { return kind == GDL_RAW_U8 ? 256 : GDL_RASTER_TONE_MAX_BINS; }

// the first k in 0..15 at which every address a + k * size of `n` (address, sample size) pairs is 16-byte aligned, or `none`
inline int64_t aligned_from(const uintptr_t* a, const size_t* size, int n, int64_t none) {
  for (int k = 0; k < 16; ++k) {
    bool all = true;
    for (int i = 0; i < n; ++i) all = all && (a[i] + k * size[i]) % 16 == 0;
    if (all) return k;
  }
  return none;
}

}  // namespace

extern "C" int gdl_raster_hist(const void* src, int kind, int C, int H, int W, const double* nodata, const uint8_t* has_nodata,
                               int bins, const double* lo, const double* hi, int64_t* acc, gdl_stream_t stream) {
  const char* fn = "gdl_raster_hist";
  if (const int bad = check_source(fn, kind, C, H, W)) return bad;
  if (kind == GDL_RAW_F32) {
    GDL_CHECK_ARG(bins >= 1 && bins <= GDL_RASTER_TONE_MAX_BINS, "%s: bins %d: a float32 histogram takes 1..%d bins", fn, bins, GDL_RASTER_TONE_MAX_BINS);
    GDL_CHECK_ARG(lo && hi, "%s: a float32 histogram needs lo and hi per band", fn);
    for (int c = 0; c < C; ++c)
      GDL_CHECK_ARG(isfinite(lo[c]) && isfinite(hi[c]) && isfinite(hi[c] - lo[c]) && lo[c] < hi[c],
                    "%s: band %d: lo %g and hi %g must be finite with lo < hi", fn, c, lo[c], hi[c]);
  } else {
    GDL_CHECK_ARG(bins == 0 || bins == kind_bins(kind), "%s: bins %d: kind %d has %d bins (or pass 0)", fn, bins, kind, kind_bins(kind));
    GDL_CHECK_ARG(!lo && !hi, "%s: lo and hi are for float32 alone: the bins of kind %d are fixed", fn, kind);
    bins = kind_bins(kind);
  }
  GDL_CHECK_ARG(src && acc, "%s: null pointer", fn);
  GDL_CHECK_ARG((uintptr_t)src % kind_size(kind) == 0 && (uintptr_t)acc % 8 == 0, "%s: src must be aligned to its samples and acc to 8 bytes", fn);
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const size_t size = kind_size(kind);
  const int vec = 16 / (int)size;
  for (int c = 0; c < C; ++c) {
    const NoData nd = band_nodata(nodata, has_nodata, c);
    const uintptr_t at = (uintptr_t)src + (uintptr_t)c * HW * size;
    const int head = (int)aligned_from(&at, &size, 1, 0);      // `at` is a multiple of the sample size: always found
    const int64_t nvec = (HW - (head < HW ? head : HW)) / vec;
    int64_t* band = acc + (int64_t)c * (bins + 2);
#define HIST(S, WORDS, COPIES, USED)                                                                                                  \
  {                                                                                                                                    \
    const int64_t runs = (nvec + HIST_THREADS * hist_iters<S>() - 1) / (HIST_THREADS * hist_iters<S>());                                         \
    const int64_t cap = (COPIES) > 1 ? 2 * HIST_GRID : HIST_GRID;                                                                      \
    const FloatBins fb = kind == GDL_RAW_F32 ? FloatBins{lo[c], hi[c], hi[c] - lo[c], (double)bins} : FloatBins{0.0, 0.0, 0.0, 0.0};   \
    hipLaunchKernelGGL((raster_hist_kernel<S, WORDS, COPIES>), dim3((unsigned)(runs < 1 ? 1 : (runs > cap ? cap : runs))),             \
                       dim3(HIST_THREADS), 0, s, (const S*)src + c * HW, HW, (int)(head < HW ? head : HW), nd, fb, USED, band);         \
  }
    if (kind == GDL_RAW_U8) HIST(uint8_t, 128, 16, 128)
    else if (kind == GDL_RAW_U16) HIST(uint16_t, HIST_WORDS, 1, GDL_RASTER_TONE_MAX_BINS / 2)
    else if (kind == GDL_RAW_I16) HIST(int16_t, HIST_WORDS, 1, GDL_RASTER_TONE_MAX_BINS / 2)
    else HIST(float, HIST_WORDS, 1, (bins + 3) / 2)
#undef HIST
  }
  GDL_CHECK_LAUNCH(fn);
  return GDL_OK;
}

extern "C" int gdl_raster_hist_quantiles(const int64_t* acc, int C, int bins, const double* q, int Q, const double* origin,
                                         const double* step, double* out, gdl_stream_t stream) {
  const char* fn = "gdl_raster_hist_quantiles";
  GDL_CHECK_ARG(C > 0 && C <= 65535, "%s: C %d must be in 1..65535", fn, C);
  GDL_CHECK_ARG(bins >= 1 && bins <= GDL_RASTER_TONE_MAX_BINS, "%s: bins %d must be in 1..%d", fn, bins, GDL_RASTER_TONE_MAX_BINS);
  GDL_CHECK_ARG(Q >= 1 && Q <= GDL_RASTER_TONE_MAX_Q, "%s: Q %d: 1..%d quantiles per call", fn, Q, GDL_RASTER_TONE_MAX_Q);
  GDL_CHECK_ARG(acc && q && origin && step && out, "%s: null pointer", fn);
  GDL_CHECK_ARG((uintptr_t)acc % 8 == 0 && (uintptr_t)out % 8 == 0, "%s: acc and out must be 8-byte aligned", fn);
  Quantiles qs{};
  for (int j = 0; j < Q; ++j) {
    GDL_CHECK_ARG(q[j] >= 0.0 && q[j] <= 1.0, "%s: q[%d] = %g is not in [0, 1]", fn, j, q[j]);
    qs.q[j] = q[j];
  }
  for (int c = 0; c < C; ++c)
    GDL_CHECK_ARG(isfinite(origin[c]) && isfinite(step[c]), "%s: band %d: origin %g and step %g must be finite", fn, c, origin[c], step[c]);
  hipStream_t s = (hipStream_t)stream;
  for (int c = 0; c < C; ++c)
    hipLaunchKernelGGL(raster_quantiles_kernel, dim3(1), dim3(QUANT_THREADS), 0, s, acc + (int64_t)c * (bins + 2), bins, qs, Q,
                       origin[c], step[c], out + (int64_t)c * Q);
  GDL_CHECK_LAUNCH(fn);
  return GDL_OK;
}

extern "C" int gdl_raster_stretch(const void* src, int kind, int C, int H, int W, const double* nodata, const uint8_t* has_nodata,
                                  const double* bounds, double out_lo, double out_hi, double dst_nodata, void* dst, int dst_kind,
                                  uint8_t* valid, gdl_stream_t stream) {
  const char* fn = "gdl_raster_stretch";
  if (const int bad = check_source(fn, kind, C, H, W)) return bad;
  GDL_CHECK_ARG(dst_kind == GDL_RAW_U8 || dst_kind == GDL_RAW_F32, "%s: the destination is uint8 or float32, got kind %d", fn, dst_kind);
  GDL_CHECK_ARG(isfinite(out_lo) && isfinite(out_hi), "%s: out_lo %g and out_hi %g must be finite", fn, out_lo, out_hi);
  if (dst_kind == GDL_RAW_U8) {
    GDL_CHECK_ARG(out_lo >= 0.0 && out_lo <= 255.0 && out_hi >= 0.0 && out_hi <= 255.0, "%s: out_lo %g and out_hi %g must lie in 0..255 for a uint8 destination", fn, out_lo, out_hi);
    GDL_CHECK_ARG(dst_nodata >= 0.0 && dst_nodata <= 255.0 && dst_nodata == floor(dst_nodata), "%s: dst_nodata %g is not a value of uint8", fn, dst_nodata);
  } else {
    GDL_CHECK_ARG(!isfinite(dst_nodata) || fabs(dst_nodata) <= FLT_MAX, "%s: dst_nodata %g is beyond float32", fn, dst_nodata);
  }
  GDL_CHECK_ARG(src && dst && bounds, "%s: null pointer", fn);
  GDL_CHECK_ARG((uintptr_t)bounds % 8 == 0, "%s: bounds must be 8-byte aligned", fn);
  GDL_CHECK_ARG((uintptr_t)src % kind_size(kind) == 0 && (uintptr_t)dst % kind_size(dst_kind) == 0, "%s: src and dst must be aligned to their samples", fn);
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const double out_span = out_hi - out_lo;
  const size_t sizes[3] = {kind_size(kind), kind_size(dst_kind), 1};
  for (int c = 0; c < C; ++c) {
    const NoData nd = band_nodata(nodata, has_nodata, c);
    const uintptr_t at[3] = {(uintptr_t)src + (uintptr_t)c * HW * sizes[0], (uintptr_t)dst + (uintptr_t)c * HW * sizes[1],
                             (uintptr_t)valid + (uintptr_t)c * HW};
    int64_t head = aligned_from(at, sizes, valid ? 3 : 2, HW);      // no common alignment: the whole band sample by sample
    head = head < HW ? head : HW;
    uint8_t* vp = valid ? valid + c * HW : nullptr;
    const int64_t work = (HW - head) / STRETCH_UNIT + 2 * STRETCH_UNIT;
    const dim3 grid(grid_for(head == HW ? HW : work));
#define STRETCH(S, D)                                                                                                                 \
  hipLaunchKernelGGL((raster_stretch_kernel<S, D>), grid, dim3(256), 0, s, (const S*)src + c * HW, HW, head, nd, bounds + 2 * c,       \
                     out_lo, out_span, (D)dst_nodata, (D*)dst + c * HW, vp);
#define STRETCH_KIND(S)                                  \
  if (dst_kind == GDL_RAW_U8) { STRETCH(S, uint8_t) }    \
  else { STRETCH(S, float) }
    if (kind == GDL_RAW_U8) { STRETCH_KIND(uint8_t) }
    else if (kind == GDL_RAW_U16) { STRETCH_KIND(uint16_t) }
    else if (kind == GDL_RAW_I16) { STRETCH_KIND(int16_t) }
    else { STRETCH_KIND(float) }
#undef STRETCH_KIND
#undef STRETCH
  }
  GDL_CHECK_LAUNCH(fn);
  return GDL_OK;
}
