// Lovasz loss (multiclass: Lovasz-Softmax, binary: Lovasz hinge): smp 0.5.0 LovaszLoss (losses/lovasz.py: _lovasz_softmax_flat,
// _lovasz_hinge_flat, _lovasz_grad), on a segmented stable radix sort written here (no library sort).
//
// A segment is the n errors of one class (per_image: of one class of one image), sorted by error, descending, ties by ascending
// flat index (torch.sort(descending=True, stable=True)).  At rank r (0-based), with the label bit z_r, G = sum z, P_r = sum_{j<=r} z_j,
// N_r = (r + 1) - P_r, I_r = G - P_r, U_r = G + N_r -- all exact u32 counts -- the Jaccard coefficient is
//   g_r = 1 / U_r (z_r = 1),   g_r = I_r / ((U_r - 1) U_r) (z_r = 0),   G = 0: g_0 = 1, every other g_r = 0
// (J_r - J_{r-1} without the cancellation), and the segment's loss is L = sum_r e_(r) g_r.
//   multiclass  p = softmax(x), z = [y == c], e = |z - p_c|; loss = mean of L_c over the classes with G_c > 0 (0 without one);
//               dL_c/de_i = g_rank(i), de/dp = -1 (z = 1) / +1 (z = 0), exactly 0 where e == 0, then back through the softmax:
//               dlogits_k = sum_c s_ic g_ic p_ic (delta_ck - p_ik) * upstream * grad_scale * norm
//   binary      z = [y == 1], s = 2z - 1, e = max(0, 1 - x s) (one rounding); dL/dx_i = -s g_rank(i) where e_i > 0, else exactly 0
// A pixel with y == ignore (int64 compare) gets key 0 and label bit 0 and an exactly zero gradient: zero keys sort behind every
// positive key and add nothing, so no compaction pass is needed.  The target is only ever compared, never used as an index.
// per_image: the mean over images of each image's mean over its present classes (binary: of each image's loss).
//
// Kernels (256 threads; wave64).  Every dependency between workgroups is a kernel boundary: no look-back, no flag, no spin.
//   keys      fused softmax -> key e + 0.0f (never -0) and payload (flat index | z << 31) per (segment, element)
//   sort      LSD radix, 8-bit digits, 4 passes over the raw bit pattern (keys >= 0), tile = 2048 elements per workgroup, the
//             segment on grid.y.  Per pass: radix_hist (per-workgroup digit histogram -> table[segment][digit][workgroup]),
//             an exclusive scan of the table (scan_apply alone up to 2048 entries; otherwise scan_reduce, scan_spine, scan_apply)
//             and radix_scatter (stable: ranks from wave ballots, waves and 256-element chunks in order).  Descending order comes
//             from the digit 255 - d, so equal keys keep ascending index order.
//   counts    lovasz_count (label bits per tile), scan_spine (exclusive tile offsets, G), lovasz_coef (P_r by ballot prefix,
//             g_r in f64 from the exact counts, e g into an f64 partial per tile, g scattered back to pixel order for the backward)
//   loss      lovasz_segsum (one workgroup per segment adds its tile partials in a fixed order), lovasz_final (present-class
//             divisor formed ON THE DEVICE, loss, and norm[segment] for the backward).  No float atomics: same input, same bits.
//   backward  recomputes the softmax from the saved logits and reads g in pixel order and norm[segment].
// A given shape always gets the same launch sequence and nothing synchronises with the host: the step captures into a hipGraph.
#include "gdl_common.h"

namespace {

constexpr int RADIX_BITS = 8, RADIX = 1 << RADIX_BITS, SORT_PASSES = 4;
constexpr int SORT_THREADS = 256, SORT_ITEMS = 8, SORT_TILE = SORT_THREADS * SORT_ITEMS;      // 2048 keys per workgroup
constexpr uint32_t LABEL_BIT = 0x80000000u, INDEX_MASK = 0x7fffffffu;

// the digit that sorts DESCENDING under an ascending stable counting sort
__device__ __forceinline__ int desc_digit(uint32_t bits, int shift) { return (RADIX - 1) - (int)((bits >> shift) & (RADIX - 1)); }

#include "scan_u32.h"      // block256_excl_scan, SCAN_TILE and the scan_reduce / scan_spine / scan_apply kernels

// ------------------------------------------------------------------ radix sort passes, grid (nwg, S)
// table[(segment * 256 + digit) * nwg + workgroup] = the number of the tile's keys with that digit
__global__ __launch_bounds__(256) void radix_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int shift,
                                                         uint32_t* __restrict__ table) {
  __shared__ uint32_t hist[RADIX];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t* seg = keys + (int64_t)blockIdx.y * n;
  const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    if (i < n) atomicAdd(&hist[desc_digit(seg[i], shift)], 1u);
  }
  __syncthreads();
  table[((int64_t)blockIdx.y * RADIX + threadIdx.x) * gridDim.x + blockIdx.x] = hist[threadIdx.x];
}

// `table` scanned: the first output slot of (digit, workgroup).  Chunks of 256 keys in index order; inside a chunk the rank of a
// key among the keys with its digit = (those in earlier waves) + (those in earlier lanes of its wave, from eight ballots).
// vals_in null: the payload is the key's index in the segment.
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                                                            uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out, int64_t n,
                                                            int shift, const uint32_t* __restrict__ table) {
  __shared__ uint32_t base[RADIX];
  __shared__ uint32_t wcount[4][RADIX];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t so = (int64_t)blockIdx.y * n, first = (int64_t)blockIdx.x * SORT_TILE;
  base[t] = table[((int64_t)blockIdx.y * RADIX + t) * gridDim.x + blockIdx.x];
#pragma unroll
  for (int w = 0; w < 4; ++w) wcount[w][t] = 0;
  uint32_t key[SORT_ITEMS], val[SORT_ITEMS];
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    const int64_t i = first + j * 256 + t;
    key[j] = i < n ? keys_in[so + i] : 0u;
    val[j] = i < n ? (vals_in ? vals_in[so + i] : (uint32_t)i) : 0u;
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    const bool valid = first + j * 256 + t < n;
    const int d = desc_digit(key[j], shift);
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < RADIX_BITS; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long set = __ballot(valid && bit);
      peers &= bit ? set : ~set;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & below);
    if (valid && rank == 0) wcount[wave][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      uint32_t pos = base[d] + rank;
#pragma unroll
      for (int w = 0; w < 4; ++w) pos += w < wave ? wcount[w][d] : 0u;
      if (pos < (uint32_t)n) {      // always true for a consistent table; keeps a stray value inside the segment
        keys_out[so + pos] = key[j];
        vals_out[so + pos] = val[j];
      }
    }
    __syncthreads();
    base[t] += wcount[0][t] + wcount[1][t] + wcount[2][t] + wcount[3][t];      // column t belongs to thread t
#pragma unroll
    for (int w = 0; w < 4; ++w) wcount[w][t] = 0;
    __syncthreads();
  }
}

// ------------------------------------------------------------------ keys
struct LovaszOpt {
  int per_image;
  int has_ignore;
  int64_t ignore;
};

__device__ __forceinline__ bool lovasz_valid(int64_t t, const LovaszOpt& o) { return !(o.has_ignore && t == o.ignore); }

// the flat position of (image b, class c, pixel p) in the [segment][element] arrays: per_image [B][K][HW] (the logits' own
// layout), otherwise [K][B * HW]
__device__ __forceinline__ int64_t lovasz_at(int b, int c, int64_t p, int B, int K, int64_t HW, int per_image) {
  return per_image ? ((int64_t)b * K + c) * HW + p : ((int64_t)c * B + b) * HW + p;
}

// max and sum exp(x - max) of the pixel's K logits
__device__ __forceinline__ void softmax_stats(const float* __restrict__ px, int K, int64_t HW, float& mx, float& sum) {
  mx = px[0];
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, px[(int64_t)k * HW]);
  sum = 0.f;
  for (int k = 0; k < K; ++k) sum += expf(px[(int64_t)k * HW] - mx);
}
__device__ __forceinline__ float softmax_at(float x, float mx, float sum) { return expf(x - mx) / sum; }
// e = |z - p| from the side that does not cancel
__device__ __forceinline__ float lovasz_err(float p, bool z) { return (z ? 1.f - p : p) + 0.0f; }

__global__ __launch_bounds__(256) void lovasz_keys_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B, int K,
                                                          int64_t HW, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                          const LovaszOpt o) {
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = target[i];
    const bool valid = lovasz_valid(t, o);
    const int b = (int)(i / HW);
    const int64_t p = i - (int64_t)b * HW;
    const float* px = logits + (int64_t)b * K * HW + p;
    float mx, sum;
    softmax_stats(px, K, HW, mx, sum);
    const uint32_t idx = (uint32_t)(o.per_image ? p : i);
    for (int k = 0; k < K; ++k) {
      const bool z = valid && t == (int64_t)k;
      const float e = valid ? lovasz_err(softmax_at(px[(int64_t)k * HW], mx, sum), z) : 0.f;
      const int64_t at = lovasz_at(b, k, p, B, K, HW, o.per_image);
      keys[at] = __float_as_uint(e);
      vals[at] = idx | (z ? LABEL_BIT : 0u);
    }
  }
}

__device__ __forceinline__ float hinge_err(float x, bool z) { return fmaxf(fmaf(z ? -1.f : 1.f, x, 1.f), 0.f) + 0.0f; }

// binary: `segs` segments of `per` logits each
__global__ __launch_bounds__(256) void lovasz_binary_keys_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                 int64_t total, int64_t per, uint32_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ vals, const LovaszOpt o) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = target[i];
    const bool valid = lovasz_valid(t, o), z = valid && t == 1;
    keys[i] = __float_as_uint(valid ? hinge_err(logits[i], z) : 0.f);
    vals[i] = (uint32_t)(i % per) | (z ? LABEL_BIT : 0u);
  }
}

// ------------------------------------------------------------------ counts, coefficients, loss.  grid (ntiles, S)
__global__ __launch_bounds__(256) void lovasz_count_kernel(const uint32_t* __restrict__ vals, int64_t n, uint32_t* __restrict__ tcount) {
  __shared__ uint32_t wsum[4];
  const uint32_t* seg = vals + (int64_t)blockIdx.y * n;
  const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
  uint32_t acc = 0;
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    acc += i < n ? seg[i] >> 31 : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) tcount[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// toff = the exclusive tile offsets of the label counts, G[segment] = the segment's positives.  coef[segment][index] = g_rank(index),
// partial[segment][tile] = sum e g of the tile (f64; wave sums, then the four waves, in a fixed order)
__global__ __launch_bounds__(256) void lovasz_coef_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t n,
                                                          const uint32_t* __restrict__ toff, const uint32_t* __restrict__ Gs,
                                                          float* __restrict__ coef, double* __restrict__ partial) {
  __shared__ uint32_t wt[SORT_ITEMS][4];
  __shared__ double red[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t so = (int64_t)blockIdx.y * n, first = (int64_t)blockIdx.x * SORT_TILE;
  const uint32_t G = Gs[blockIdx.y];
  const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
  uint32_t key[SORT_ITEMS], val[SORT_ITEMS], inc[SORT_ITEMS];
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    const int64_t i = first + j * 256 + t;
    key[j] = i < n ? keys[so + i] : 0u;
    val[j] = i < n ? vals[so + i] : 0u;
    const unsigned long long ones = __ballot((val[j] & LABEL_BIT) != 0);
    inc[j] = (uint32_t)__popcll(ones & upto);
    if (lane == 0) wt[j][wave] = (uint32_t)__popcll(ones);
  }
  __syncthreads();
  uint32_t off = toff[(int64_t)blockIdx.y * gridDim.x + blockIdx.x];
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < SORT_ITEMS; ++j) {
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      before += w < wave ? wt[j][w] : 0u;
      all += wt[j][w];
    }
    const int64_t r = first + j * 256 + t;
    if (r < n) {
      const bool z = (val[j] & LABEL_BIT) != 0;
      const uint32_t P = off + before + inc[j];                 // inclusive count of positives
      const double I = (double)(G - P), U = (double)G + (double)((uint32_t)(r + 1) - P);
      const double g = G == 0 ? (r == 0 ? 1.0 : 0.0) : (z ? 1.0 / U : I / ((U - 1.0) * U));
      acc += (double)__uint_as_float(key[j]) * g;
      const uint32_t idx = val[j] & INDEX_MASK;
      if (idx < (uint32_t)n) coef[so + idx] = (float)g;      // always true: the payload is an index into the segment
    }
    off += all;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (t == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// grid S: segloss[segment] = the sum of its nt tile partials (strided per thread, then a tree)
__global__ __launch_bounds__(256) void lovasz_segsum_kernel(const double* __restrict__ partial, int64_t nt, double* __restrict__ segloss) {
  __shared__ double part[256];
  const double* seg = partial + (int64_t)blockIdx.x * nt;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < nt; i += 256) acc += seg[i];
  part[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) segloss[blockIdx.x] = part[0];
}

// one workgroup.  Segments = nimg images x K classes.  An image's loss = the mean of its classes' losses over the classes counted
// (only_present: those with G > 0, 0 without one; otherwise all K), the loss = the mean over images.  norm[segment] = the weight
// of the segment's loss in that mean (0 for a class that is not counted): what the backward multiplies into the coefficients.
__global__ __launch_bounds__(256) void lovasz_final_kernel(const double* __restrict__ segloss, const uint32_t* __restrict__ Gs, int nimg,
                                                           int K, int only_present, float* __restrict__ loss, float* __restrict__ norm) {
  __shared__ double part[256];
  double acc = 0.0;
  for (int b = threadIdx.x; b < nimg; b += 256) {
    int counted = 0;
    double sum = 0.0;
    for (int c = 0; c < K; ++c) {
      const bool in = !only_present || Gs[(int64_t)b * K + c] > 0;
      counted += in;
      sum += in ? segloss[(int64_t)b * K + c] : 0.0;
    }
    const double w = counted ? 1.0 / ((double)counted * (double)nimg) : 0.0;
    for (int c = 0; c < K; ++c) norm[(int64_t)b * K + c] = !only_present || Gs[(int64_t)b * K + c] > 0 ? (float)w : 0.f;
    acc += sum * w;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)part[0];
}

// ------------------------------------------------------------------ backward
__global__ __launch_bounds__(256) void lovasz_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B, int K,
                                                         int64_t HW, const float* __restrict__ coef, const float* __restrict__ norm,
                                                         const float* __restrict__ upstream, float scale, float* __restrict__ dlogits,
                                                         int accumulate, const LovaszOpt o) {
  const float up = (upstream ? upstream[0] : 1.f) * scale;
  const int64_t total = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = target[i];
    const bool valid = lovasz_valid(t, o);
    const int b = (int)(i / HW);
    const int64_t p = i - (int64_t)b * HW;
    const float* px = logits + (int64_t)b * K * HW + p;
    float* pd = dlogits + (int64_t)b * K * HW + p;
    float mx = 0.f, sum = 1.f, dot = 0.f;
    if (valid) {
      softmax_stats(px, K, HW, mx, sum);
      // w_c = dL/dp_c: -g (z = 1) / +g (z = 0), times the segment's weight; exactly 0 where e == 0.  dot = sum_c w_c p_c
      for (int k = 0; k < K; ++k) {
        const bool z = t == (int64_t)k;
        const float pk = softmax_at(px[(int64_t)k * HW], mx, sum);
        const float g = coef[lovasz_at(b, k, p, B, K, HW, o.per_image)] * norm[o.per_image ? b * K + k : k];
        const float w = lovasz_err(pk, z) == 0.f ? 0.f : (z ? -g : g);
        dot += w * pk;
      }
    }
    for (int k = 0; k < K; ++k) {
      const int64_t at = (int64_t)k * HW;
      float v = 0.f;      // an ignored pixel: exactly zero
      if (valid) {
        const bool z = t == (int64_t)k;
        const float pk = softmax_at(px[at], mx, sum);
        const float g = coef[lovasz_at(b, k, p, B, K, HW, o.per_image)] * norm[o.per_image ? b * K + k : k];
        const float w = lovasz_err(pk, z) == 0.f ? 0.f : (z ? -g : g);
        v = up * pk * (w - dot);
      }
      pd[at] = accumulate ? pd[at] + v : v;
    }
  }
}

__global__ __launch_bounds__(256) void lovasz_binary_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                int64_t total, int64_t per, const float* __restrict__ coef,
                                                                const float* __restrict__ norm, const float* __restrict__ upstream,
                                                                float scale, float* __restrict__ dlogits, int accumulate,
                                                                const LovaszOpt o) {
  const float up = (upstream ? upstream[0] : 1.f) * scale;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = target[i];
    const bool valid = lovasz_valid(t, o), z = valid && t == 1;
    float v = 0.f;
    if (valid && hinge_err(logits[i], z) > 0.f) {
      const float g = up * coef[i] * norm[i / per];
      v = z ? -g : g;
    }
    dlogits[i] = accumulate ? dlogits[i] + v : v;
  }
}

// ------------------------------------------------------------------ host
inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }
inline int64_t tiles_of(int64_t n) { return (n + SORT_TILE - 1) / SORT_TILE; }
inline int64_t scan_blocks(int64_t L) { return (L + SCAN_TILE - 1) / SCAN_TILE; }

// what one sort needs beside its key / payload buffers
struct SortScratch {
  uint32_t* table;      // [S][256][nwg]
  uint32_t* bsum;       // [S][nb]
};
inline int64_t table_bytes(int S, int64_t n) { return align256((int64_t)S * RADIX * tiles_of(n) * 4); }
inline int64_t bsum_bytes(int S, int64_t n) { return align256((int64_t)S * scan_blocks(RADIX * tiles_of(n)) * 4); }

bool sort_shape_ok(int S, int64_t n) { return S >= 1 && S <= 65535 && n >= 1 && n < ((int64_t)1 << 31) && tiles_of(n) <= 0x7fffffff / RADIX; }

// keys / payloads in a -> sorted into a (through b); a's payload null on entry: the index
void radix_sort_desc(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_a, uint32_t* vals_a, uint32_t* keys_b,
                     uint32_t* vals_b, const SortScratch& sc, int S, int64_t n, hipStream_t s) {
  const int64_t nwg = tiles_of(n), L = RADIX * nwg, nb = scan_blocks(L);
  const dim3 grid((unsigned)nwg, (unsigned)S), sgrid((unsigned)nb, (unsigned)S);
  for (int pass = 0; pass < SORT_PASSES; ++pass) {
    const uint32_t* kin = pass == 0 ? keys_in : (pass & 1 ? keys_b : keys_a);
    const uint32_t* vin = pass == 0 ? vals_in : (pass & 1 ? vals_b : vals_a);
    uint32_t* kout = pass & 1 ? keys_a : keys_b;
    uint32_t* vout = pass & 1 ? vals_a : vals_b;
    const int shift = pass * RADIX_BITS;
    hipLaunchKernelGGL(radix_hist_kernel, grid, dim3(256), 0, s, kin, n, shift, sc.table);
    if (nb > 1) {
      hipLaunchKernelGGL(scan_reduce_kernel, sgrid, dim3(256), 0, s, (const uint32_t*)sc.table, L, sc.bsum);
      hipLaunchKernelGGL(scan_spine_kernel, dim3((unsigned)S), dim3(256), 0, s, sc.bsum, nb, (uint32_t*)nullptr);
    }
    hipLaunchKernelGGL(scan_apply_kernel, sgrid, dim3(256), 0, s, sc.table, L, nb > 1 ? (const uint32_t*)sc.bsum : (const uint32_t*)nullptr);
    hipLaunchKernelGGL(radix_scatter_kernel, grid, dim3(256), 0, s, kin, vin, kout, vout, n, shift, (const uint32_t*)sc.table);
  }
}

// the workspace of the losses, carved in this order
struct LovaszWs {
  uint32_t *keys_a, *vals_a, *keys_b, *vals_b;
  SortScratch sc;
  uint32_t *tcount, *G;
  double *partial, *segloss;
};
int64_t lovasz_carve(void* ws, int S, int64_t n, LovaszWs* out) {
  const int64_t nt = tiles_of(n), kv = align256((int64_t)S * n * 4);
  const int64_t sizes[10] = {kv, kv, kv, kv, table_bytes(S, n), bsum_bytes(S, n), align256((int64_t)S * nt * 4), align256((int64_t)S * 4),
                             align256((int64_t)S * nt * 8), align256((int64_t)S * 8)};
  char* p = (char*)ws;
  void* at[10];
  int64_t total = 0;
  for (int i = 0; i < 10; ++i) {
    at[i] = p + total;
    total += sizes[i];
  }
  if (out) {
    out->keys_a = (uint32_t*)at[0]; out->vals_a = (uint32_t*)at[1]; out->keys_b = (uint32_t*)at[2]; out->vals_b = (uint32_t*)at[3];
    out->sc.table = (uint32_t*)at[4]; out->sc.bsum = (uint32_t*)at[5];
    out->tcount = (uint32_t*)at[6]; out->G = (uint32_t*)at[7];
    out->partial = (double*)at[8]; out->segloss = (double*)at[9];
  }
  return total;
}

// keys and payloads are in w.keys_a / w.vals_a: sort, count, coefficients, loss
void lovasz_after_keys(const LovaszWs& w, int nimg, int K, int64_t n, int only_present, float* loss, float* coef, float* norm, hipStream_t s) {
  const int S = nimg * K;
  const int64_t nt = tiles_of(n);
  const dim3 grid((unsigned)nt, (unsigned)S);
  radix_sort_desc(w.keys_a, w.vals_a, w.keys_a, w.vals_a, w.keys_b, w.vals_b, w.sc, S, n, s);
  hipLaunchKernelGGL(lovasz_count_kernel, grid, dim3(256), 0, s, (const uint32_t*)w.vals_a, n, w.tcount);
  hipLaunchKernelGGL(scan_spine_kernel, dim3((unsigned)S), dim3(256), 0, s, w.tcount, nt, w.G);
  hipLaunchKernelGGL(lovasz_coef_kernel, grid, dim3(256), 0, s, (const uint32_t*)w.keys_a, (const uint32_t*)w.vals_a, n,
                     (const uint32_t*)w.tcount, (const uint32_t*)w.G, coef, w.partial);
  hipLaunchKernelGGL(lovasz_segsum_kernel, dim3((unsigned)S), dim3(256), 0, s, (const double*)w.partial, nt, w.segloss);
  hipLaunchKernelGGL(lovasz_final_kernel, dim3(1), dim3(256), 0, s, (const double*)w.segloss, (const uint32_t*)w.G, nimg, K, only_present,
                     loss, norm);
}

}  // namespace

// ============================================================================ C ABI
extern "C" int64_t gdl_sort_desc_workspace(int S, int64_t n) {
  if (!sort_shape_ok(S, n)) return 0;
  return 2 * align256((int64_t)S * n * 4) + table_bytes(S, n) + bsum_bytes(S, n);
}

extern "C" int gdl_sort_desc_f32(const float* keys, int S, int64_t n, float* sorted, int32_t* perm, void* ws, int64_t ws_bytes,
                                 gdl_stream_t stream) {
  GDL_CHECK_ARG(keys && sorted && perm && ws, "gdl_sort_desc_f32: null pointer");
  GDL_CHECK_ARG(sort_shape_ok(S, n), "gdl_sort_desc_f32: bad sizes (1 <= S <= 65535 segments of 1 <= n < 2^31 keys)");
  GDL_CHECK_ARG(ws_bytes >= gdl_sort_desc_workspace(S, n) && (uintptr_t)ws % 8 == 0, "gdl_sort_desc_f32: workspace too small or misaligned");
  const int64_t kv = align256((int64_t)S * n * 4);
  char* p = (char*)ws;
  SortScratch sc{(uint32_t*)(p + 2 * kv), (uint32_t*)(p + 2 * kv + table_bytes(S, n))};
  radix_sort_desc((const uint32_t*)keys, nullptr, (uint32_t*)sorted, (uint32_t*)perm, (uint32_t*)p, (uint32_t*)(p + kv), sc, S, n,
                  (hipStream_t)stream);
  GDL_CHECK_LAUNCH("gdl_sort_desc_f32");
  return GDL_OK;
}

extern "C" int64_t gdl_lovasz_workspace(int S, int64_t n, int K) {
  if (!sort_shape_ok(S, n) || K < 1 || S % K != 0) return 0;
  return lovasz_carve(nullptr, S, n, nullptr);
}

#define LOVASZ_OPT() \
  LovaszOpt o;       \
  o.per_image = per_image != 0; o.has_ignore = has_ignore != 0; o.ignore = ignore

extern "C" int gdl_lovasz_fwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, int per_image, int has_ignore,
                              int64_t ignore, float* loss, float* coef, float* norm, void* ws, int64_t ws_bytes, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && loss && coef && norm && ws, "gdl_lovasz_fwd: null pointer");
  GDL_CHECK_ARG(B > 0 && K >= 1 && HW > 0 && (int64_t)B * K <= 65535 && (int64_t)B * HW < ((int64_t)1 << 31),
                "gdl_lovasz_fwd: bad sizes (B=%d K=%d HW=%lld)", B, K, (long long)HW);
  const int nimg = per_image ? B : 1;
  const int S = nimg * K;
  const int64_t n = per_image ? HW : (int64_t)B * HW;
  GDL_CHECK_ARG(sort_shape_ok(S, n), "gdl_lovasz_fwd: bad sizes");
  GDL_CHECK_ARG(ws_bytes >= gdl_lovasz_workspace(S, n, K) && (uintptr_t)ws % 8 == 0, "gdl_lovasz_fwd: workspace too small or misaligned");
  LOVASZ_OPT();
  LovaszWs w;
  lovasz_carve(ws, S, n, &w);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lovasz_keys_kernel, dim3(grid_for((int64_t)B * HW)), dim3(256), 0, s, logits, target, B, K, HW, w.keys_a, w.vals_a, o);
  lovasz_after_keys(w, nimg, K, n, 1, loss, coef, norm, s);
  GDL_CHECK_LAUNCH("gdl_lovasz_fwd");
  return GDL_OK;
}

extern "C" int gdl_lovasz_bwd(const float* logits, const int64_t* target, int B, int K, int64_t HW, int per_image, int has_ignore,
                              int64_t ignore, const float* coef, const float* norm, const float* upstream, float grad_scale,
                              float* dlogits, int accumulate, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && coef && norm && dlogits, "gdl_lovasz_bwd: null pointer");
  GDL_CHECK_ARG(B > 0 && K >= 1 && HW > 0 && (int64_t)B * K <= 65535 && (int64_t)B * HW < ((int64_t)1 << 31),
                "gdl_lovasz_bwd: bad sizes (B=%d K=%d HW=%lld)", B, K, (long long)HW);
  LOVASZ_OPT();
  hipLaunchKernelGGL(lovasz_bwd_kernel, dim3(grid_for((int64_t)B * HW)), dim3(256), 0, (hipStream_t)stream, logits, target, B, K, HW, coef,
                     norm, upstream, grad_scale, dlogits, accumulate, o);
  GDL_CHECK_LAUNCH("gdl_lovasz_bwd");
  return GDL_OK;
}

// ---- binary: B images of `per` logits each; per_image: one segment per image, otherwise one segment of B * per
extern "C" int gdl_lovasz_binary_fwd(const float* logits, const int64_t* target, int B, int64_t per, int per_image, int has_ignore,
                                     int64_t ignore, float* loss, float* coef, float* norm, void* ws, int64_t ws_bytes,
                                     gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && loss && coef && norm && ws, "gdl_lovasz_binary_fwd: null pointer");
  GDL_CHECK_ARG(B > 0 && per > 0 && B <= 65535 && (int64_t)B * per < ((int64_t)1 << 31), "gdl_lovasz_binary_fwd: bad sizes (B=%d per=%lld)", B,
                (long long)per);
  const int S = per_image ? B : 1;
  const int64_t n = per_image ? per : (int64_t)B * per;
  GDL_CHECK_ARG(ws_bytes >= gdl_lovasz_workspace(S, n, 1) && (uintptr_t)ws % 8 == 0, "gdl_lovasz_binary_fwd: workspace too small or misaligned");
  LOVASZ_OPT();
  LovaszWs w;
  lovasz_carve(ws, S, n, &w);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lovasz_binary_keys_kernel, dim3(grid_for((int64_t)B * per)), dim3(256), 0, s, logits, target, (int64_t)B * per, n,
                     w.keys_a, w.vals_a, o);
  lovasz_after_keys(w, S, 1, n, 0, loss, coef, norm, s);
  GDL_CHECK_LAUNCH("gdl_lovasz_binary_fwd");
  return GDL_OK;
}

extern "C" int gdl_lovasz_binary_bwd(const float* logits, const int64_t* target, int B, int64_t per, int per_image, int has_ignore,
                                     int64_t ignore, const float* coef, const float* norm, const float* upstream, float grad_scale,
                                     float* dlogits, int accumulate, gdl_stream_t stream) {
  GDL_CHECK_ARG(logits && target && coef && norm && dlogits, "gdl_lovasz_binary_bwd: null pointer");
  GDL_CHECK_ARG(B > 0 && per > 0 && B <= 65535 && (int64_t)B * per < ((int64_t)1 << 31), "gdl_lovasz_binary_bwd: bad sizes (B=%d per=%lld)", B,
                (long long)per);
  LOVASZ_OPT();
  const int64_t n = per_image ? per : (int64_t)B * per;
  hipLaunchKernelGGL(lovasz_binary_bwd_kernel, dim3(grid_for((int64_t)B * per)), dim3(256), 0, (hipStream_t)stream, logits, target,
                     (int64_t)B * per, n, coef, norm, upstream, grad_scale, dlogits, accumulate, o);
  GDL_CHECK_LAUNCH("gdl_lovasz_binary_bwd");
  return GDL_OK;
}
