// The last kernel of a forward whose mean divides by a sum formed on the device (loss_focal.hip: the number of valid pixels;
// loss_xent.hip: the summed class weights of the valid pixels).  Included only by the files that launch it: a __global__ function
// is emitted into every translation unit that sees its definition.
#pragma once
#include "gdl_common.h"

namespace {

// one workgroup: the two sums of n partials each in a fixed order (strided per thread, then a tree); the divisor
// (mean: 1 / the second sum, 0 where that is not positive; sum: 1) -> norm[0], loss = the first sum * divisor
__global__ __launch_bounds__(256) void mean_final_kernel(const double* __restrict__ ws, int n, int mean, float* __restrict__ loss,
                                                         float* __restrict__ norm) {
  __shared__ double part[256], pcnt[256];
  const int t = threadIdx.x;
  double acc = 0.0, cnt = 0.0;
#pragma unroll 8
  for (int i = t; i < n; i += 256) acc += ws[i];
#pragma unroll 8
  for (int i = t; i < n; i += 256) cnt += ws[n + i];
  part[t] = acc;
  pcnt[t] = cnt;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      part[t] += part[t + s];
      pcnt[t] += pcnt[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double inv = mean ? (pcnt[0] > 0.0 ? 1.0 / pcnt[0] : 0.0) : 1.0;
    loss[0] = (float)(part[0] * inv);
    norm[0] = (float)inv;
  }
}

}  // namespace
