// Elementwise and packing kernels with no subject of their own: casts, scales, broadcast row adds, the eval-mode BatchNorm fold
// and the forward -> data-gradient weight repack.  A kernel that belongs to a model stage goes to that stage's unit, not here.
#include "gdl_common.h"

namespace {

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void cast_kernel(const void* __restrict__ in, void* out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    ElemIO<TO>::store(out, i, ElemIO<TI>::load(in, i));
}

__global__ __launch_bounds__(256) void scale_f32_kernel(const float* __restrict__ in, float* out, int64_t n, float s) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = in[i] * s;
}

// out[r,:] = a[(r % a_rows),:] + (b ? b[(r % b_rows),:] : 0)
__global__ __launch_bounds__(256) void add_rows_kernel(const float* __restrict__ a, int64_t a_rows, int64_t a_stride,
                                                       const float* __restrict__ b, int64_t b_rows, int64_t b_stride,
                                                       float* out, int64_t out_stride, int64_t rows, int D) {
  const int64_t total = rows * D;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / D;
    const int c = (int)(i - r * D);
    float v = a[(r % a_rows) * a_stride + c];
    if (b) v += b[(r % b_rows) * b_stride + c];
    out[r * out_stride + c] = v;
  }
}

// x[o, r, :] *= s[o]   (DropPath: o = sample; Dropout2d on NHWC handled via chan_scale elsewhere)
template <typename T>
__global__ __launch_bounds__(256) void scale_outer_kernel(void* x, const float* __restrict__ s, int64_t outer, int64_t inner) {
  const int64_t total = outer * inner;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    ElemIO<T>::store(x, i, ElemIO<T>::load(x, i) * s[i / inner]);
}

// eval-mode BatchNorm folded into the conv epilogue: scale = g*rsqrt(var+eps), shift = b - mean*scale
__global__ void bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                               const float* __restrict__ mean, const float* __restrict__ var, float eps, int C,
                               float* __restrict__ scale, float* __restrict__ shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float s = gamma[c] / sqrtf(var[c] + eps);
  scale[c] = s;
  shift[c] = beta[c] - mean[c] * s;
}

// forward weights [N][T][C] (T = R*S taps) -> data-gradient weights [C][T][N] with the taps flipped
// (t' = T-1-t): dx = conv(dy, w_dgrad, pad = R-1-pad).  32x32 LDS tile transpose per tap.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void pack_dgrad_kernel(const void* __restrict__ w, int N, int T, int Cc,
                                                         void* out) {
  __shared__ float tile[32][33];
  const int t = blockIdx.z, n0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8) {
    const int n = n0 + j, c = c0 + tx;
    tile[j][tx] = (n < N && c < Cc) ? ElemIO<TI>::load(w, ((int64_t)n * T + t) * Cc + c) : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j, n = n0 + tx;
    if (c < Cc && n < N) ElemIO<TO>::store(out, ((int64_t)c * T + (T - 1 - t)) * N + n, tile[tx][j]);
  }
}

}  // namespace

extern "C" int gdl_cast(const void* in, int in_dtype, void* out, int out_dtype, int64_t n, gdl_stream_t stream) {
  GDL_CHECK_ARG(in && out, "gdl_cast: null pointer");
  if (n <= 0) return GDL_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(grid_for(n));
  if (in_dtype == GDL_F32 && out_dtype == GDL_BF16) hipLaunchKernelGGL((cast_kernel<float, bf16_tag>), grid, dim3(256), 0, s, in, out, n);
  else if (in_dtype == GDL_BF16 && out_dtype == GDL_F32) hipLaunchKernelGGL((cast_kernel<bf16_tag, float>), grid, dim3(256), 0, s, in, out, n);
  else if (in_dtype == GDL_F32) hipLaunchKernelGGL((cast_kernel<float, float>), grid, dim3(256), 0, s, in, out, n);
  else hipLaunchKernelGGL((cast_kernel<bf16_tag, bf16_tag>), grid, dim3(256), 0, s, in, out, n);
  GDL_CHECK_LAUNCH("gdl_cast");
  return GDL_OK;
}

extern "C" int gdl_scale_f32(const float* in, float* out, int64_t n, float s, gdl_stream_t stream) {
  GDL_CHECK_ARG(in && out, "gdl_scale_f32: null pointer");
  if (n <= 0) return GDL_OK;
  hipLaunchKernelGGL(scale_f32_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, out, n, s);
  GDL_CHECK_LAUNCH("gdl_scale_f32");
  return GDL_OK;
}

extern "C" int gdl_add_rows(const float* a, int64_t a_rows, int64_t a_stride, const float* b, int64_t b_rows,
                            int64_t b_stride, float* out, int64_t out_stride, int64_t rows, int D,
                            gdl_stream_t stream) {
  GDL_CHECK_ARG(a && out && a_rows > 0 && (!b || b_rows > 0), "gdl_add_rows: bad args");
  hipLaunchKernelGGL(add_rows_kernel, dim3(grid_for(rows * D)), dim3(256), 0, (hipStream_t)stream, a, a_rows, a_stride, b,
                     b_rows, b_stride, out, out_stride, rows, D);
  GDL_CHECK_LAUNCH("gdl_add_rows");
  return GDL_OK;
}

extern "C" int gdl_scale_outer(void* x, int dtype, const float* s, int64_t outer, int64_t inner, gdl_stream_t stream) {
  GDL_CHECK_ARG(x && s, "gdl_scale_outer: null pointer");
  const int64_t total = outer * inner;
  if (total <= 0) return GDL_OK;
  if (dtype == GDL_BF16) hipLaunchKernelGGL(scale_outer_kernel<bf16_tag>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, s, outer, inner);
  else hipLaunchKernelGGL(scale_outer_kernel<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, s, outer, inner);
  GDL_CHECK_LAUNCH("gdl_scale_outer");
  return GDL_OK;
}

extern "C" int gdl_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                           int C, float* scale, float* shift, gdl_stream_t stream) {
  GDL_CHECK_ARG(gamma && beta && mean && var && scale && shift, "gdl_bn_fold: null pointer");
  hipLaunchKernelGGL(bn_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, gamma, beta, mean, var, eps, C, scale, shift);
  GDL_CHECK_LAUNCH("gdl_bn_fold");
  return GDL_OK;
}

extern "C" int gdl_pack_dgrad(const void* w, int w_dtype, int N, int T, int C, void* out, int out_dtype,
                              gdl_stream_t stream) {
  GDL_CHECK_ARG(w && out && N > 0 && T > 0 && C > 0, "gdl_pack_dgrad: bad args");
  dim3 grid((C + 31) / 32, (N + 31) / 32, T);
  hipStream_t s = (hipStream_t)stream;
  if (w_dtype == GDL_F32 && out_dtype == GDL_BF16) hipLaunchKernelGGL((pack_dgrad_kernel<float, bf16_tag>), grid, dim3(256), 0, s, w, N, T, C, out);
  else if (w_dtype == GDL_F32) hipLaunchKernelGGL((pack_dgrad_kernel<float, float>), grid, dim3(256), 0, s, w, N, T, C, out);
  else if (out_dtype == GDL_BF16) hipLaunchKernelGGL((pack_dgrad_kernel<bf16_tag, bf16_tag>), grid, dim3(256), 0, s, w, N, T, C, out);
  else hipLaunchKernelGGL((pack_dgrad_kernel<bf16_tag, float>), grid, dim3(256), 0, s, w, N, T, C, out);
  GDL_CHECK_LAUNCH("gdl_pack_dgrad");
  return GDL_OK;
}
