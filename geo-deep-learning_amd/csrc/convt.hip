// Operand layouts of nn.ConvTranspose2d(kernel_size=2, stride=2) (UperNet scale_modules, models/decoders/upernet.py:37-54).
//
// Kernel = stride, so no output pixel receives two taps:
//     out[b, 2y + py, 2x + px, n] = bias[n] + sum_c in[b, y, x, c] * w[c][n][py][px]
// and the layer is the adjoint of a 2x2 / stride-2 convolution.  All three GEMMs run on the existing MFMA entry points:
//   forward  gdl_conv_gemm, nz = 4 phases of a 1x1 problem, weight [Cout][Cin] per phase, phase-strided output;
//   dgrad    gdl_conv_gemm on dy with R = S = 2, stride 2, weight [Cin][(py,px,n)];
//   wgrad    gdl_conv_wgrad with in = dy (R = S = 2, stride 2) and dy = x  ->  f32 [Cin][(py,px,n)].
// The kernels here only move the parameter between torch's [Cin][Cout][2][2] and those layouts: one launch builds both GEMM
// operands from the f32 parameter, one launch turns the weight-gradient GEMM's result into the parameter's gradient.
#include "gdl_common.h"

namespace {

constexpr int CT_TILE = 32;      // cin x cout tile of one workgroup

// w [Cin][Cout][4] f32 -> fwd [4][Cout][Cin] and dgrad [Cin][4 * Cout], both of dtype T.  A workgroup owns a 32 x 32 (cin, cout)
// tile: 16-byte loads along cout (coalesced), the dgrad rows are written on the way (cout-contiguous), the forward operand after
// a turn through LDS (cin-contiguous).
template <typename T>
__global__ __launch_bounds__(256) void convt2x2_pack_kernel(const float* __restrict__ w, int Cin, int Cout, void* fwd, void* dgrad) {
  __shared__ float tile[4][CT_TILE][CT_TILE + 1];      // [phase][cout][cin]
  const int ci0 = blockIdx.y * CT_TILE, co0 = blockIdx.x * CT_TILE;
  for (int i = threadIdx.x; i < CT_TILE * CT_TILE; i += 256) {
    const int lci = i / CT_TILE, lco = i % CT_TILE;
    const int ci = ci0 + lci, co = co0 + lco;
    if (ci < Cin && co < Cout) {
      const float4 v = *(const float4*)(w + ((int64_t)ci * Cout + co) * 4);
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int ph = 0; ph < 4; ++ph) {
        tile[ph][lco][lci] = e[ph];
        ElemIO<T>::store(dgrad, (int64_t)ci * 4 * Cout + (int64_t)ph * Cout + co, e[ph]);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * CT_TILE * CT_TILE; i += 256) {
    const int lci = i % CT_TILE, lco = (i / CT_TILE) % CT_TILE, ph = i / (CT_TILE * CT_TILE);
    const int ci = ci0 + lci, co = co0 + lco;
    if (ci < Cin && co < Cout) ElemIO<T>::store(fwd, ((int64_t)ph * Cout + co) * Cin + ci, tile[ph][lco][lci]);
  }
}

// dw [Cin][4 * Cout] f32 (the weight-gradient GEMM's layout) -> grad [Cin][Cout][4] f32 (+= when accumulate): one thread per
// (cin, cout), four loads that are contiguous along cout across the wave, one 16-byte store
__global__ __launch_bounds__(256) void convt2x2_unpack_grad_kernel(const float* __restrict__ dw, int Cin, int Cout, float* grad,
                                                                   int accumulate) {
  const int64_t total = (int64_t)Cin * Cout;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t ci = i / Cout;
    const int co = (int)(i - ci * Cout);
    const float* src = dw + ci * 4 * Cout + co;
    float4 v = make_float4(src[0], src[Cout], src[2 * (int64_t)Cout], src[3 * (int64_t)Cout]);
    float4* dst = (float4*)(grad + i * 4);
    if (accumulate) {
      const float4 o = *dst;
      v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
    }
    *dst = v;
  }
}

}  // namespace

extern "C" int gdl_convt2x2_pack(const float* w, int Cin, int Cout, int out_dtype, void* fwd, void* dgrad, gdl_stream_t stream) {
  GDL_CHECK_ARG(w && fwd && dgrad && Cin > 0 && Cout > 0, "gdl_convt2x2_pack: bad args");
  GDL_CHECK_ARG(out_dtype == GDL_F32 || out_dtype == GDL_BF16, "gdl_convt2x2_pack: bad out_dtype");
  GDL_CHECK_ARG((uintptr_t)w % 16 == 0, "gdl_convt2x2_pack: the parameter must be 16-byte aligned");
  const dim3 grid((Cout + CT_TILE - 1) / CT_TILE, (Cin + CT_TILE - 1) / CT_TILE);
  GDL_CHECK_ARG(grid.y <= 65535, "gdl_convt2x2_pack: Cin too large");
  if (out_dtype == GDL_BF16)
    hipLaunchKernelGGL(convt2x2_pack_kernel<bf16_tag>, grid, dim3(256), 0, (hipStream_t)stream, w, Cin, Cout, fwd, dgrad);
  else
    hipLaunchKernelGGL(convt2x2_pack_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, w, Cin, Cout, fwd, dgrad);
  GDL_CHECK_LAUNCH("gdl_convt2x2_pack");
  return GDL_OK;
}

extern "C" int gdl_convt2x2_unpack_grad(const float* dw, int Cin, int Cout, float* grad, int accumulate, gdl_stream_t stream) {
  GDL_CHECK_ARG(dw && grad && Cin > 0 && Cout > 0, "gdl_convt2x2_unpack_grad: bad args");
  GDL_CHECK_ARG((uintptr_t)grad % 16 == 0, "gdl_convt2x2_unpack_grad: the gradient must be 16-byte aligned");
  int64_t blocks = ((int64_t)Cin * Cout + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(convt2x2_unpack_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dw, Cin, Cout, grad,
                     accumulate);
  GDL_CHECK_LAUNCH("gdl_convt2x2_unpack_grad");
  return GDL_OK;
}
