// Exclusive scan of S arrays of L u32, in place, in three launches (256 threads; wave64): shared by loss_lovasz.hip (the radix
// sort's digit table, the label counts; it issues the launches itself and skips the first two for a single block) and, through
// scan_exclusive below, by scene_rings.hip (the boundary sides per pixel, the ring starts and vertex counts), scene_simplify.hip
// (the dense positions, the anchors, the kept vertices), scene_regions.hip (the root flags) and scene_burn.hip (the rows per edge).
//   scan_reduce  grid (nb, S), nb = ceil(L / SCAN_TILE): the sum of every block of SCAN_TILE entries -> bsum[segment][block]
//   scan_spine   grid (S): the exclusive prefix of a segment's block sums in place, and their total
//   scan_apply   grid (nb, S): the exclusive scan of a block's entries plus the block's offset
// Every dependency between workgroups is a kernel boundary.  Include inside the file's anonymous namespace, after gdl_common.h.
#pragma once

constexpr int SCAN_TILE = 2048;                                                               // table entries per scan workgroup

// exclusive prefix of v over the 256 threads of the workgroup, the workgroup's total in `total`.  `wsum`: 4 LDS words.
__device__ __forceinline__ uint32_t block256_excl_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();      // wsum may still be read from an earlier call
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) before += w < wave ? wsum[w] : 0u;
  total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return before + inc - v;
}

// ------------------------------------------------------------------ exclusive scan of S arrays of L u32 (in place)
// block sums: grid (nb, S)
__global__ __launch_bounds__(256) void scan_reduce_kernel(const uint32_t* __restrict__ data, int64_t L, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t wsum[4];
  const uint32_t* seg = data + (int64_t)blockIdx.y * L;
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
  uint32_t acc = 0;
#pragma unroll
  for (int j = 0; j < SCAN_TILE / 256; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    acc += i < L ? seg[i] : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) bsum[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup per segment: sums[segment][0 .. m) -> their exclusive prefix in place, the sum of all in total[segment] (may be null)
__global__ __launch_bounds__(256) void scan_spine_kernel(uint32_t* __restrict__ sums, int64_t m, uint32_t* __restrict__ total) {
  __shared__ uint32_t wsum[4];
  uint32_t* seg = sums + (int64_t)blockIdx.x * m;
  uint32_t carry = 0;
  for (int64_t c = 0; c < m; c += 256) {
    const int64_t i = c + threadIdx.x;
    const uint32_t v = i < m ? seg[i] : 0u;
    uint32_t tot;
    const uint32_t ex = block256_excl_scan(v, wsum, tot);
    if (i < m) seg[i] = carry + ex;
    carry += tot;
  }
  if (total && threadIdx.x == 0) total[blockIdx.x] = carry;
}

// grid (nb, S): the exclusive scan of the block's SCAN_TILE entries plus the block's offset (bsum null: one block, offset 0)
__global__ __launch_bounds__(256) void scan_apply_kernel(uint32_t* __restrict__ data, int64_t L, const uint32_t* __restrict__ bsum) {
  __shared__ uint32_t wsum[4];
  uint32_t* seg = data + (int64_t)blockIdx.y * L;
  const int64_t first = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * (SCAN_TILE / 256);
  uint32_t v[SCAN_TILE / 256], mine = 0;
#pragma unroll
  for (int j = 0; j < SCAN_TILE / 256; ++j) {
    v[j] = first + j < L ? seg[first + j] : 0u;
    mine += v[j];
  }
  uint32_t tot;
  uint32_t run = block256_excl_scan(mine, wsum, tot) + (bsum ? bsum[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] : 0u);
#pragma unroll
  for (int j = 0; j < SCAN_TILE / 256; ++j) {
    if (first + j < L) seg[first + j] = run;
    run += v[j];
  }
}

// the exclusive scan of S arrays of L u32 in place, their totals in total[S] (may be null); bsum: S * ceil(L / SCAN_TILE) words
void scan_exclusive(uint32_t* data, int S, int64_t L, uint32_t* bsum, uint32_t* total, hipStream_t s) {
  const int64_t nb = (L + SCAN_TILE - 1) / SCAN_TILE;      // L <= 2^31: at most 2^20 blocks
  const dim3 grid((unsigned)nb, (unsigned)S);
  hipLaunchKernelGGL(scan_reduce_kernel, grid, dim3(256), 0, s, (const uint32_t*)data, L, bsum);
  hipLaunchKernelGGL(scan_spine_kernel, dim3((unsigned)S), dim3(256), 0, s, bsum, nb, total);
  hipLaunchKernelGGL(scan_apply_kernel, grid, dim3(256), 0, s, data, L, (const uint32_t*)bsum);
}
