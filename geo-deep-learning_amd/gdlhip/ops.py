"""Tensor-level wrappers over the C-ABI (raw ops, no autograd).

Conventions: activations are NHWC torch tensors ``[B, H, W, C]`` (any strides with
``stride(-1) == 1``); 2-D ``[rows, C]`` tensors are treated as ``[1, 1, rows, C]``.
PyTorch only provides device memory and the stream here -- all arithmetic happens in
libgdlhip.so.  Shape / dtype / alignment errors raise ValueError like the reference's own
argument checks (dofa_v2.py:439-441, multilevel_neck.py:141-146).
"""

from __future__ import annotations

import ctypes as C
import math
import os
from typing import NamedTuple

import torch
from torch import Tensor

from . import _lib
from ._lib import (ACT_GELU, ACT_MUL_GELU_GRAD, ACT_NONE, ACT_RELU, ACT_RESID_RELU, BF16, F32, ConvArgs,  # noqa: F401
                   WgradArgs, check)

_DT = {torch.float32: F32, torch.bfloat16: BF16}


def dt(t: Tensor | torch.dtype) -> int:
    d = t if isinstance(t, torch.dtype) else t.dtype
    try:
        return _DT[d]
    except KeyError:
        raise ValueError(f"gdlhip: unsupported dtype {d}") from None


def _p(t: Tensor | None):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(*ts: Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("gdlhip ops need CUDA/HIP device tensors (no CPU fallback)")


def _f32vec(t: Tensor | None, n: int, name: str) -> Tensor | None:
    if t is None:
        return None
    if t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous f32 vector of {n} elements")
    return t


def image_f32(img: Tensor, who: str) -> Tensor:
    """Model-entry check: tiles must arrive normalised (floating point).  A raw integer tile would silently train on
    0..255 pixels -- the reference never sees one (its workers normalise, wds_dataset.py:230-236); here raw tiles are
    only legal upstream of DeviceInputStage / normalize_raw."""
    if not img.is_floating_point():
        raise TypeError(f"{who}: image dtype {img.dtype} is a raw tile; normalise it first (DeviceInputStage, "
                        f"gdlhip.ops.normalize_raw or the host path of SampleProcessor)")
    return img.float().contiguous()


def as_nhwc(x: Tensor) -> Tensor:
    """Logical NCHW tensor -> NHWC view (copying only if its channels are not contiguous)."""
    v = x.permute(0, 2, 3, 1)
    return v if v.stride(-1) == 1 else v.contiguous()


def as_nchw(x: Tensor) -> Tensor:
    """NHWC tensor -> logical NCHW view (== torch.channels_last memory format)."""
    return x.permute(0, 3, 1, 2)


def _nhwc4(x: Tensor, name: str) -> Tensor:
    if x.dim() == 2:
        x = x.unsqueeze(0).unsqueeze(0)
    if x.dim() != 4 or (x.stride(-1) != 1 and x.shape[-1] != 1):
        raise ValueError(f"{name}: expected NHWC tensor with unit channel stride, got "
                         f"shape {tuple(x.shape)} strides {x.stride()}")
    # strides of size-1 dims are arbitrary in torch: canonicalise them (alignment checks, "dense" tests)
    B, H, W, Cc = x.shape
    sB, sH, sW, _ = x.stride()
    nW = sW if W > 1 else Cc
    nH = sH if H > 1 else W * nW
    nB = sB if B > 1 else H * nH
    if (nB, nH, nW) != (sB, sH, sW) or x.stride(-1) != 1:
        x = x.as_strided((B, H, W, Cc), (nB, nH, nW, 1))
    return x


# ------------------------------------------------------------------ conv / linear (MFMA)
def conv_gemm(x: Tensor, w: Tensor, *, R: int = 1, S: int = 1, stride: int = 1, pad: int = 0,
              bias: Tensor | None = None, scale: Tensor | None = None, shift: Tensor | None = None,
              act: int = ACT_NONE, batch_scale: Tensor | None = None, resid: Tensor | None = None,
              out: Tensor | None = None, out_dtype: torch.dtype | None = None,
              alpha: float = 1.0, aux_out: Tensor | None = None, want_stats: bool = False):
    """out = epilogue(conv(x, w)); x NHWC [B,H,W,C], w [N, R*S*C] (K order r,s,c).
    ``aux_out`` (same shape / dtype / strides as out) receives the pre-activation values.
    ``want_stats``: returns (out, partials, rows) -- when the call can emit them (gdl_conv_gemm_stats_rows: bf16, bias-only
    epilogue, whole tiles) `partials` [rows, 2, N] f32 holds per-channel sums and sums of squares of the bf16 outputs for
    bn_stats_finalize (train-mode BatchNorm statistics without a pass over `out`); otherwise (out, None, 0)."""
    _need_cuda(x, w)
    two_d = x.dim() == 2
    x4 = _nhwc4(x, "conv_gemm input")
    B, H, W, Cc = x4.shape
    N = w.shape[0]
    if w.dim() != 2 or w.shape[1] != R * S * Cc or w.stride(1) != 1 or w.dtype != x.dtype:
        raise ValueError(f"conv_gemm: weight must be [{N}, {R * S * Cc}] {x.dtype} K-contiguous, "
                         f"got {tuple(w.shape)} {w.dtype}")
    Ho = (H + 2 * pad - R) // stride + 1
    Wo = (W + 2 * pad - S) // stride + 1
    if out is None:
        out = torch.empty((B, Ho, Wo, N), device=x.device, dtype=out_dtype or x.dtype)
        out4 = out
    else:
        out4 = _nhwc4(out, "conv_gemm out")
        if tuple(out4.shape) != (B, Ho, Wo, N):
            raise ValueError(f"conv_gemm: out shape {tuple(out4.shape)} != {(B, Ho, Wo, N)}")
    a = ConvArgs()
    a.inp, a.dtype = x4.data_ptr(), dt(x)
    a.B, a.H, a.W, a.C = B, H, W, Cc
    a.in_sB, a.in_sH, a.in_sW = x4.stride(0), x4.stride(1), x4.stride(2)
    a.Ho, a.Wo, a.R, a.S, a.stride, a.pad = Ho, Wo, R, S, stride, pad
    a.w, a.w_sN, a.N = w.data_ptr(), w.stride(0), N
    a.out, a.out_dtype = out4.data_ptr(), dt(out4)
    a.out_sB, a.out_sH, a.out_sW = out4.stride(0), out4.stride(1), out4.stride(2)
    a.alpha = alpha
    a.bias = None if bias is None else _f32vec(bias, N, "bias").data_ptr()
    a.scale = None if scale is None else _f32vec(scale, N, "scale").data_ptr()
    a.shift = None if shift is None else _f32vec(shift, N, "shift").data_ptr()
    a.act = act
    a.batch_scale = None if batch_scale is None else _f32vec(batch_scale, B, "batch_scale").data_ptr()
    if resid is not None:
        r4 = _nhwc4(resid, "conv_gemm resid")
        if r4.shape[-1] != N or r4.shape[1:3] != out4.shape[1:3]:
            raise ValueError("conv_gemm: resid shape mismatch")
        a.resid, a.resid_dtype = r4.data_ptr(), dt(r4)
        a.res_sB = r4.stride(0) if r4.shape[0] == B else 0
        a.res_sH, a.res_sW = r4.stride(1), r4.stride(2)
    if aux_out is not None:
        x4a = _nhwc4(aux_out, "conv_gemm aux_out")
        if x4a.shape != out4.shape or x4a.stride() != out4.stride() or x4a.dtype != out4.dtype:
            raise ValueError("conv_gemm: aux_out must match out in shape, strides and dtype")
        a.aux_out = x4a.data_ptr()
    a.nz, a.nz_inner = 1, 1
    partials, rows = None, 0
    if want_stats:
        rows = int(_lib.load().gdl_conv_gemm_stats_rows(C.byref(a)))
        if rows:
            partials = torch.empty((rows, 2, N), device=x.device, dtype=torch.float32)
            a.stats_partial = partials.data_ptr()
    _launch_conv_gemm(a, "gdl_conv_gemm")
    if two_d and out4 is out:
        out = out.view(Wo, N)
    return (out, partials, rows) if want_stats else out


class KernelTimer:
    """HIP-event timing of every gdl_conv_gemm launch (bench.py's roofline leg).  Events are
    recorded on the stream the kernels are launched on (torch's current stream)."""

    VARIANT = {0: "conv_gemm_kernel<{dt},2,2,1,1> (64x64 tiles)", 1: "conv_gemm_kernel<{dt},2,2,2,2> (128x128 tiles)",
               2: "conv_gemm_kernel<{dt},2,4,4,2> (256x256 tiles)",
               3: "conv_gemm_kernel<{dt},2,4,4,2,pingpong> (256x256 tiles, alternating loader halves)",
               4: "conv3x3_sf_kernel<{dt}> (256x256 tiles, 3x3 taps share one staged activation tile)",
               5: "conv_gemm_kernel<{dt},4,1,2,2> (256x64 tiles, narrow outputs)",
               6: "conv_gemm_dual_kernel (256x128 tiles, four waves, two workgroups resident per CU)",
               8: "conv_gemm_w4_kernel (256x256 tiles, one wave per SIMD, every load in an MFMA shadow)",
               9: "conv_gemm_persist_kernel (256x256 ping-pong tiles, one persistent workgroup per CU, next tile's first stage under the epilogue)",
               10: "conv_gemm_w4p_kernel (256x256 tiles, one persistent workgroup per CU, one wave per SIMD, finished tile parked in registers and stored from the next tile's MFMA shadows)",
               7: "conv3x3_narrow_kernel (direct 3x3, C <= 32, one staged window per 4 x 64 pixels x 32 output channels)",
               12: "conv_gemm_kernel<{dt},2,2,1,1,stages=4> (64x64 tiles, four LDS stages: few tiles, long K)"}

    def __init__(self) -> None:
        self.records: list = []
        self.variants: list = []      # the planner's tile variant of every launch, in launch order

    def launch(self, a: ConvArgs, what: str) -> None:
        lib = _lib.load()
        fl = C.c_int64()
        variant = lib.gdl_conv_gemm_plan(C.byref(a), C.byref(fl))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        status = lib.gdl_conv_gemm(C.byref(a), _stream())
        e1.record()
        check(status, what)
        key = self.VARIANT[variant].format(dt="bf16" if a.dtype == BF16 else "f32")
        # algorithmic bytes of the launch: every operand read once, the result written once, at their dtypes
        es, oes = (2 if a.dtype == BF16 else 4), (2 if a.out_dtype == BF16 else 4)
        nz = int(a.nz)
        nbytes = nz * (int(a.B) * int(a.H) * int(a.W) * int(a.C) * es + int(a.N) * int(a.R) * int(a.S) * int(a.C) * es
                       + int(a.B) * int(a.Ho) * int(a.Wo) * int(a.N) * oes)
        if a.resid:
            nbytes += nz * int(a.B) * int(a.Ho) * int(a.Wo) * int(a.N) * (2 if a.resid_dtype == BF16 else 4)
        shape = (nz * int(a.B) * int(a.Ho) * int(a.Wo), int(a.N), int(a.R) * int(a.S) * int(a.C), int(a.R), int(a.S), oes, bool(a.resid))
        self.records.append((key, fl.value, e0, e1, int(a.R) * int(a.S) * int(a.C), nbytes, shape))
        self.variants.append(variant)

    @staticmethod
    def _k_bucket(k: int) -> str:
        return "K<=1024" if k <= 1024 else ("1024<K<=4096" if k <= 4096 else "K>4096")

    def summary(self) -> dict:
        """Per kernel class: launches, ms, flops, and the same split by reduction depth K = R*S*C (`by_k`): one class runs
        12-K-step ViT linears and 100-K-step convolutions, whose achievable rates differ by a factor of two."""
        torch.cuda.synchronize()
        out: dict = {}
        for key, flops, e0, e1, kdepth, nbytes, shape in self.records:
            ms = e0.elapsed_time(e1)
            s = out.setdefault(key, {"launches": 0, "ms": 0.0, "flops": 0, "bytes": 0, "by_k": {}, "by_shape": {}})
            m_, n_, k_, r_, s_, oes, res = shape
            tag = f"M{m_} N{n_} K{k_} {r_}x{s_} -> {'bf16' if oes == 2 else 'f32'}{' +resid' if res else ''}"
            for d in (s, s["by_k"].setdefault(self._k_bucket(kdepth), {"launches": 0, "ms": 0.0, "flops": 0, "bytes": 0}),
                      s["by_shape"].setdefault(tag, {"launches": 0, "ms": 0.0, "flops": 0, "bytes": 0})):
                d["launches"] += 1
                d["ms"] += ms
                d["flops"] += flops
                d["bytes"] += nbytes
        return out


TIMER: KernelTimer | None = None


def _launch_conv_gemm(a: ConvArgs, what: str) -> None:
    if TIMER is not None:
        TIMER.launch(a, what)
    else:
        check(_lib.load().gdl_conv_gemm(C.byref(a), _stream()), what)


def linear(x: Tensor, w: Tensor, bias: Tensor | None = None, **kw) -> Tensor:
    """y[..., N] = epilogue(x[..., K] @ w[N, K]^T); rows may be strided."""
    K = x.shape[-1]
    lead = x.shape[:-1]
    x2 = x.reshape(-1, K)
    if "resid" in kw and kw["resid"] is not None:
        kw["resid"] = kw["resid"].reshape(-1, w.shape[0])
    for key in ("out", "aux_out"):
        if kw.get(key) is not None:
            kw[key] = kw[key].reshape(-1, w.shape[0])
    y = conv_gemm(x2, w, bias=bias, **kw)
    return y.reshape(*lead, w.shape[0])


def batched_gemm_raw(a: ConvArgs) -> None:
    _launch_conv_gemm(a, "gdl_conv_gemm(batched)")


def conv_gemm_grouped(x: Tensor, w: Tensor, *, R: int, S: int, stride: int = 1, pad: int = 0, out: Tensor | None = None) -> Tensor:
    """Grouped convolution as ONE batched implicit-GEMM launch: x NHWC [B,H,W,Z*c], w [Z, n, R*S*c] (K order r,s,c) -> out
    [B,Ho,Wo,Z*n]; problem z reads channels z*c.. of x with filter w[z] and writes channels z*n.. of out (grid.z = z: the
    operands are channel slices addressed through the batch strides of gdl_conv_args, nothing is copied).  No epilogue terms:
    per-channel vectors are not offset per z by the kernels."""
    _need_cuda(x, w)
    x4 = _nhwc4(x, "conv_gemm_grouped input")
    B, H, W, Ct = x4.shape
    Z, n, kk = w.shape
    c = kk // (R * S)
    if w.dim() != 3 or c * R * S != kk or Z * c != Ct or not w.is_contiguous() or w.dtype != x.dtype:
        raise ValueError(f"conv_gemm_grouped: weight must be contiguous [Z, n, {R * S}*c] {x.dtype} with Z*c = {Ct}, got {tuple(w.shape)} {w.dtype}")
    Ho = (H + 2 * pad - R) // stride + 1
    Wo = (W + 2 * pad - S) // stride + 1
    if out is None:
        out = torch.empty((B, Ho, Wo, Z * n), device=x.device, dtype=x.dtype)
    o4 = _nhwc4(out, "conv_gemm_grouped out")
    if tuple(o4.shape) != (B, Ho, Wo, Z * n):
        raise ValueError(f"conv_gemm_grouped: out shape {tuple(o4.shape)} != {(B, Ho, Wo, Z * n)}")
    a = ConvArgs()
    a.inp, a.dtype = x4.data_ptr(), dt(x4)
    a.B, a.H, a.W, a.C = B, H, W, c
    a.in_sB, a.in_sH, a.in_sW = x4.stride(0), x4.stride(1), x4.stride(2)
    a.Ho, a.Wo, a.R, a.S, a.stride, a.pad = Ho, Wo, R, S, stride, pad
    a.w, a.w_sN, a.N = w.data_ptr(), kk, n
    a.out, a.out_dtype = o4.data_ptr(), dt(o4)
    a.out_sB, a.out_sH, a.out_sW = o4.stride(0), o4.stride(1), o4.stride(2)
    a.alpha, a.act = 1.0, ACT_NONE
    a.nz, a.nz_inner = Z, 1
    a.in_sZ0, a.w_sZ0, a.out_sZ0 = c, n * kk, n
    _launch_conv_gemm(a, "gdl_conv_gemm(grouped)")
    return out


def conv_wgrad_grouped(x: Tensor, dy: Tensor, *, Z: int, R: int, S: int, stride: int = 1, pad: int = 0) -> Tensor:
    """Weight gradient of conv_gemm_grouped: dw [Z, n, R*S*c] f32, problem z = channel slices z*c.. of x and z*n.. of dy."""
    _need_cuda(x, dy)
    x4, dy4 = _nhwc4(x, "wgrad x"), _nhwc4(dy, "wgrad dy")
    if x4.dtype != dy4.dtype:
        raise ValueError("conv_wgrad_grouped: x and dy dtypes differ")
    B, H, W, Ct = x4.shape
    _, Ho, Wo, Nt = dy4.shape
    if Ct % Z or Nt % Z:
        raise ValueError("conv_wgrad_grouped: channel counts must be multiples of Z")
    c, n = Ct // Z, Nt // Z
    dw = torch.empty((Z, n, R * S * c), device=x.device, dtype=torch.float32)
    a = WgradArgs()
    a.inp, a.dy, a.dtype = x4.data_ptr(), dy4.data_ptr(), dt(x4)
    a.B, a.H, a.W, a.C = B, H, W, c
    a.in_sB, a.in_sH, a.in_sW = x4.stride(0), x4.stride(1), x4.stride(2)
    a.Ho, a.Wo, a.R, a.S, a.stride, a.pad, a.N = Ho, Wo, R, S, stride, pad, n
    a.dy_sB, a.dy_sH, a.dy_sW = dy4.stride(0), dy4.stride(1), dy4.stride(2)
    a.dw, a.dw_sN, a.accumulate = dw.data_ptr(), R * S * c, 0
    a.nz, a.nz_inner = Z, 1
    a.in_sZ0, a.dy_sZ0, a.dw_sZ0 = c, n, n * R * S * c
    lib = _lib.load()
    nbytes = lib.gdl_conv_wgrad_workspace(C.byref(a))
    ws = torch.empty(max(nbytes, 4) // 4, device=x.device, dtype=torch.float32)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    check(lib.gdl_conv_wgrad(C.byref(a), _stream()), "gdl_conv_wgrad(grouped)")
    return dw


# (Round 6, measured and removed: weight gradients launched on a SIDE stream -- leaves of the backward pass, MFMA-bound, meant to
# share the chip with the HBM-bound BatchNorm-backward / gather kernels that follow on the main stream; joined by an autograd engine
# callback at the end of backward.  Three same-box A/B repetitions at batch 64: 936.5-944.1 without, 934.7-937.7 with
# (profiles/r06o_*): a GEMM-class workgroup takes a CU's whole register file and LDS, so nothing co-resides with it, and the GEMM
# phases already sit at the power cap.)
def conv_wgrad(x: Tensor, dy: Tensor, *, R: int, S: int, stride: int = 1, pad: int = 0,
               dw: Tensor | None = None, accumulate: bool = False) -> Tensor:
    """dw[N, R*S*C] (f32) = sum_pixels dy[.., n] * x[.. + tap, c]."""
    _need_cuda(x, dy)
    x4, dy4 = _nhwc4(x, "wgrad x"), _nhwc4(dy, "wgrad dy")
    if x4.dtype != dy4.dtype:
        raise ValueError("conv_wgrad: x and dy dtypes differ")
    B, H, W, Cc = x4.shape
    _, Ho, Wo, N = dy4.shape
    if dw is None:
        dw = torch.empty((N, R * S * Cc), device=x.device, dtype=torch.float32)
    a = WgradArgs()
    a.inp, a.dy, a.dtype = x4.data_ptr(), dy4.data_ptr(), dt(x4)
    a.B, a.H, a.W, a.C = B, H, W, Cc
    a.in_sB, a.in_sH, a.in_sW = x4.stride(0), x4.stride(1), x4.stride(2)
    a.Ho, a.Wo, a.R, a.S, a.stride, a.pad, a.N = Ho, Wo, R, S, stride, pad, N
    a.dy_sB, a.dy_sH, a.dy_sW = dy4.stride(0), dy4.stride(1), dy4.stride(2)
    a.dw, a.dw_sN, a.accumulate = dw.data_ptr(), dw.stride(0), int(accumulate)
    a.nz, a.nz_inner = 1, 1
    lib = _lib.checked()
    nbytes = lib.gdl_conv_wgrad_workspace(C.byref(a))
    ws = torch.empty(max(nbytes, 4) // 4, device=x.device, dtype=torch.float32)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    lib.gdl_conv_wgrad(C.byref(a), _stream())
    return dw


# ------------------------------------------------------------------ normalisation
def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, out_dtype: torch.dtype) -> Tensor:
    _need_cuda(x)
    if x.dtype != torch.float32 or x.stride(-1) != 1:
        raise ValueError("layernorm: x must be f32 with unit last stride")
    D = x.shape[-1]
    x2 = x.reshape(-1, D)
    y = torch.empty((x2.shape[0], D), device=x.device, dtype=out_dtype)
    _lib.checked().gdl_layernorm_fwd(_p(x2), x2.stride(0), _p(_f32vec(gamma, D, "gamma")),
                                     _p(_f32vec(beta, D, "beta")), _p(y), dt(y), x2.shape[0], D,
                                     eps, _stream())
    return y.reshape(x.shape)


def _pix(x: Tensor, name: str):
    """NHWC tensor whose pixels are uniformly strided -> (P, C, pixel stride)."""
    x4 = _nhwc4(x, name)
    B, H, W, Cc = x4.shape
    sB, sH, sW = x4.stride(0), x4.stride(1), x4.stride(2)
    if W > 1:
        sP = sW
    elif H > 1:
        sP = sH
    else:
        sP = sB if B > 1 else Cc
    ok = (H == 1 or W == 1 or sH == W * sP) and (B == 1 or H * W == 1 or sB == H * W * sP)
    if not ok:
        raise ValueError(f"{name}: pixels must be uniformly strided, got strides {x4.stride()}")
    return B * H * W, Cc, sP


def bn_stats(x: Tensor, running_mean: Tensor | None = None, running_var: Tensor | None = None,
             momentum: float = 0.1):
    _need_cuda(x)
    P, Cc, sP = _pix(x, "bn_stats x")
    mean = torch.empty(Cc, device=x.device, dtype=torch.float32)
    var = torch.empty_like(mean)
    lib = _lib.checked()
    nbytes = lib.gdl_bn_stats_workspace(P, Cc)
    ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32)
    lib.gdl_bn_stats(_p(x), dt(x), P, Cc, sP, _p(mean), _p(var), _p(running_mean),
                     _p(running_var), momentum, _p(ws), nbytes, _stream())
    return mean, var


def bn_stats_finalize(partials: Tensor, rows: int, channels: int, pixels: int, running_mean: Tensor | None = None,
                      running_var: Tensor | None = None, momentum: float = 0.1):
    """(mean, biased var) from [rows, 2, C] partial sums written by a producing kernel (conv_gemm(want_stats=True)); updates the
    running buffers like bn_stats."""
    _need_cuda(partials)
    mean = torch.empty(channels, device=partials.device, dtype=torch.float32)
    var = torch.empty_like(mean)
    _lib.checked().gdl_bn_stats_finalize(_p(partials), rows, channels, pixels, _p(mean), _p(var), _p(running_mean),
                                         _p(running_var), momentum, _stream())
    return mean, var


def bn_apply(x: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, beta: Tensor, eps: float,
             relu: bool, out: Tensor | None = None) -> Tensor:
    P, Cc, sP = _pix(x, "bn_apply x")
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    Po, Co, sPo = _pix(out, "bn_apply out")
    _lib.checked().gdl_bn_apply(_p(x), _p(out), dt(x), P, Cc, sP, sPo, _p(mean), _p(var),
                                _p(gamma), _p(beta), eps, int(relu), _stream())
    return out


def _syncbn_pivot(pivot: Tensor | None, c: int, what: str) -> Tensor | None:
    if pivot is not None and (pivot.numel() != c or pivot.dtype != torch.float32 or not pivot.is_contiguous()):
        raise ValueError(f"{what}: pivot must be a contiguous f32 tensor of C elements")
    return pivot


def syncbn_pack(mean: Tensor, var: Tensor, count: float, out: Tensor, pivot: Tensor | None = None) -> None:
    """With d = mean - pivot: out[0:C] = count * d, out[C:2C] = count * (var + d^2), out[2C] = count: one rank's share of the
    SyncBatchNorm message (out: a contiguous f32 slice of 2 C + 1 elements of the message buffer).  ``pivot`` [C]: values that are
    identical on every rank (the layer's running_mean), None = 0; syncbn_unpack must be given the same."""
    c = mean.numel()
    if out.numel() != 2 * c + 1 or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("syncbn_pack: out must be a contiguous f32 slice of 2 C + 1 elements")
    _lib.checked().gdl_syncbn_pack(_p(mean), _p(var), float(count), c, _p(_syncbn_pivot(pivot, c, "syncbn_pack")), _p(out), _stream())


def syncbn_unpack(packed: Tensor, channels: int, running_mean: Tensor | None = None, running_var: Tensor | None = None,
                  momentum: float = 0.1, pivot: Tensor | None = None):
    """(global mean, global biased var) from the all-reduced message slice [sum n (mean - pivot) | sum n E[(x - pivot)^2] | sum n];
    the running estimates are updated with the unbiased variance over the global count (which stays on the device).  ``pivot``: what
    syncbn_pack was given (it may be ``running_mean`` itself: it is read before the update)."""
    if packed.numel() != 2 * channels + 1 or packed.dtype != torch.float32 or not packed.is_contiguous():
        raise ValueError("syncbn_unpack: packed must be a contiguous f32 slice of 2 C + 1 elements")
    mean = torch.empty(channels, device=packed.device, dtype=torch.float32)
    var = torch.empty_like(mean)
    _lib.checked().gdl_syncbn_unpack(_p(packed), channels, _p(_syncbn_pivot(pivot, channels, "syncbn_unpack")), _p(mean), _p(var),
                                     _p(running_mean), _p(running_var), momentum, _stream())
    return mean, var


def bn_bwd_dx_sync(x, dy, mean, var, gamma, beta, eps, relu, dgamma_sum, dbeta_sum, total_count: Tensor, out: Tensor | None = None):
    """bn_bwd_dx with the all-reduced sums and the GLOBAL pixel count read from device memory (``total_count``: one f32 element,
    e.g. entry 2 C of the forward message)."""
    P, Cc, sP = _pix(x, "bn_bwd x")
    _, _, sPd = _pix(dy, "bn_bwd dy")
    dx = out if out is not None else torch.empty(x.shape, device=x.device, dtype=x.dtype)
    _, _, sPx = _pix(dx, "bn_bwd dx")
    if total_count.dtype != torch.float32 or total_count.numel() != 1:
        raise ValueError("bn_bwd_dx_sync: total_count must be one f32 element on the device")
    _lib.checked().gdl_bn_bwd_dx_sync(_p(x), _p(dy), _p(dx), dt(x), P, Cc, sP, sPd, sPx, _p(mean), _p(var), _p(gamma), _p(beta), eps,
                                      int(relu), _p(dgamma_sum), _p(dbeta_sum), _p(total_count), _stream())
    return dx


# OFF by default (0): measured at per-GPU batch 4 (profiles/r05d_*), the one-launch kernels make the EAGER step 5-10 % faster
# (fewer launches to issue) but the step replayed from a hipGraph -- the default path at that batch -- 3.8 % SLOWER (447 vs 465
# tiles/s): a workgroup that owns four channels over all pixels reads 8 bytes out of every 128-byte line, and the C / 4
# workgroups sit on different XCDs, so every line crosses the fabric up to sixteen times; the three short many-workgroup
# launches read whole lines.  GDL_BN_SMALL_PIXELS=8192 switches them on (host-bound eager loops without graph capture).
BN_SMALL_MAX_PIXELS = int(os.environ.get("GDL_BN_SMALL_PIXELS", "0"))


def bn_small_ok(x: Tensor) -> bool:
    """Maps the one-launch BatchNorm kernels take: at most BN_SMALL_MAX_PIXELS pixels (each workgroup walks ALL pixels of its
    four channels: beyond a few thousand the many-workgroup kernels win)."""
    if x.dim() < 2 or x.shape[-1] % 4:
        return False
    return 0 < x.numel() // x.shape[-1] <= BN_SMALL_MAX_PIXELS


def bn_small_fits(x: Tensor) -> bool:
    """Shapes the kernels can take at all (tests; the dispatch uses bn_small_ok)."""
    return x.dim() >= 2 and x.shape[-1] % 4 == 0 and x.numel() > 0


def bn_small_fwd(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, relu: bool, running_mean: Tensor | None = None,
                 running_var: Tensor | None = None, momentum: float = 0.1):
    """Train-mode BatchNorm(+ReLU) of a small map in ONE launch: (out, mean, biased var); updates the running buffers."""
    _need_cuda(x)
    P, Cc, sP = _pix(x, "bn_small_fwd x")
    out = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    _, _, sPo = _pix(out, "bn_small_fwd out")
    mean = torch.empty(Cc, device=x.device, dtype=torch.float32)
    var = torch.empty_like(mean)
    _lib.checked().gdl_bn_small_fwd(_p(x), _p(out), dt(x), P, Cc, sP, sPo, _p(gamma), _p(beta), eps, int(relu), _p(mean), _p(var),
                                    _p(running_mean), _p(running_var), momentum, _stream())
    return out, mean, var


def bn_small_bwd(x: Tensor, dy: Tensor, mean, var, gamma, beta, eps, relu, out: Tensor | None = None):
    """Backward of bn_small_fwd in ONE launch: (dx, dgamma, dbeta).  ``out`` may be x (dx then replaces the saved conv output)."""
    P, Cc, sP = _pix(x, "bn_small_bwd x")
    _, _, sPd = _pix(dy, "bn_small_bwd dy")
    if dy.dtype != x.dtype:
        raise ValueError("bn_small_bwd: dy dtype must match x")
    dx = out if out is not None else torch.empty(x.shape, device=x.device, dtype=x.dtype)
    _, _, sPx = _pix(dx, "bn_small_bwd dx")
    dgamma = torch.empty(Cc, device=x.device, dtype=torch.float32)
    dbeta = torch.empty_like(dgamma)
    _lib.checked().gdl_bn_small_bwd(_p(x), _p(dy), _p(dx), dt(x), P, Cc, sP, sPd, sPx, _p(mean), _p(var), _p(gamma), _p(beta), eps,
                                    int(relu), _p(dgamma), _p(dbeta), _stream())
    return dx, dgamma, dbeta


def bn_bwd_reduce(x, dy, mean, var, gamma, beta, eps, relu):
    P, Cc, sP = _pix(x, "bn_bwd x")
    _, _, sPd = _pix(dy, "bn_bwd dy")
    if dy.dtype != x.dtype:
        raise ValueError("bn_bwd: dy dtype must match x")
    dgamma = torch.empty(Cc, device=x.device, dtype=torch.float32)
    dbeta = torch.empty_like(dgamma)
    lib = _lib.checked()
    nbytes = lib.gdl_bn_stats_workspace(P, Cc)
    ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32)
    lib.gdl_bn_bwd_reduce(_p(x), _p(dy), dt(x), P, Cc, sP, sPd, _p(mean), _p(var), _p(gamma),
                          _p(beta), eps, int(relu), _p(dgamma), _p(dbeta), _p(ws), nbytes,
                          _stream())
    return dgamma, dbeta


def bn_bwd_dx(x, dy, mean, var, gamma, beta, eps, relu, dgamma_sum, dbeta_sum, p_total,
              out: Tensor | None = None):
    P, Cc, sP = _pix(x, "bn_bwd x")
    _, _, sPd = _pix(dy, "bn_bwd dy")
    dx = out if out is not None else torch.empty(x.shape, device=x.device, dtype=x.dtype)
    _, _, sPx = _pix(dx, "bn_bwd dx")
    _lib.checked().gdl_bn_bwd_dx(_p(x), _p(dy), _p(dx), dt(x), P, Cc, sP, sPd, sPx, _p(mean),
                                 _p(var), _p(gamma), _p(beta), eps, int(relu), _p(dgamma_sum),
                                 _p(dbeta_sum), p_total, _stream())
    return dx


# ------------------------------------------------------------------ BatchNorm -> GELU (UperNet scale_modules, fpn1.1 / fpn1.2)
def bn_gelu_apply(x: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, beta: Tensor, eps: float, out: Tensor | None = None) -> Tensor:
    """gelu(batch_norm(x)) (erf GELU) with the given per-channel statistics: batch statistics in training (bn_stats), running
    estimates in eval.  ``out`` may be x."""
    _need_cuda(x)
    P, Cc, sP = _pix(x, "bn_gelu_apply x")
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    _, _, sPo = _pix(out, "bn_gelu_apply out")
    _lib.checked().gdl_bn_gelu_apply(_p(x), _p(out), dt(x), P, Cc, sP, sPo, _p(_f32vec(mean, Cc, "mean")), _p(_f32vec(var, Cc, "var")),
                                     _p(_f32vec(gamma, Cc, "gamma")), _p(_f32vec(beta, Cc, "beta")), eps, _stream())
    return out


def bn_gelu_bwd_reduce(x: Tensor, dy: Tensor, mean, var, gamma, beta, eps):
    """(dgamma, dbeta) = (sum g * xhat, sum g), g = dy * gelu'(bn(x)), from the saved convolution output x."""
    _need_cuda(x, dy)
    P, Cc, sP = _pix(x, "bn_gelu_bwd x")
    _, _, sPd = _pix(dy, "bn_gelu_bwd dy")
    if dy.dtype != x.dtype or dy.shape != x.shape:
        raise ValueError("bn_gelu_bwd: dy must match x in shape and dtype")
    dgamma = torch.empty(Cc, device=x.device, dtype=torch.float32)
    dbeta = torch.empty_like(dgamma)
    lib = _lib.checked()
    nbytes = lib.gdl_bn_stats_workspace(P, Cc)
    ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32)
    lib.gdl_bn_gelu_bwd_reduce(_p(x), _p(dy), dt(x), P, Cc, sP, sPd, _p(mean), _p(var), _p(gamma), _p(beta), eps, _p(dgamma),
                               _p(dbeta), _p(ws), nbytes, _stream())
    return dgamma, dbeta


def bn_gelu_bwd_dx(x: Tensor, dy: Tensor, mean, var, gamma, beta, eps, dgamma_sum, dbeta_sum, p_total: int,
                   total_count: Tensor | None = None, out: Tensor | None = None) -> Tensor:
    """dx of gelu(batch_norm(x)) from the (all-reduced) sums; ``total_count``: the global pixel count as one f32 element on the
    device (SyncBatchNorm), else ``p_total``.  ``out`` may be x."""
    _need_cuda(x, dy)
    P, Cc, sP = _pix(x, "bn_gelu_bwd x")
    _, _, sPd = _pix(dy, "bn_gelu_bwd dy")
    if dy.dtype != x.dtype or dy.shape != x.shape:
        raise ValueError("bn_gelu_bwd: dy must match x in shape and dtype")
    dx = out if out is not None else torch.empty(x.shape, device=x.device, dtype=x.dtype)
    _, _, sPx = _pix(dx, "bn_gelu_bwd dx")
    if total_count is not None and (total_count.dtype != torch.float32 or total_count.numel() != 1):
        raise ValueError("bn_gelu_bwd_dx: total_count must be one f32 element on the device")
    _lib.checked().gdl_bn_gelu_bwd_dx(_p(x), _p(dy), _p(dx), dt(x), P, Cc, sP, sPd, sPx, _p(mean), _p(var), _p(gamma), _p(beta), eps,
                                      _p(dgamma_sum), _p(dbeta_sum), int(p_total), _p(total_count), _stream())
    return dx


# ------------------------------------------------------------------ ConvTranspose2d(kernel 2, stride 2) (UperNet scale_modules)
def _convt_channels(cin: int, cout: int, dtype: torch.dtype) -> None:
    al = 8 if dtype == torch.bfloat16 else 4
    if cin % al or cout % al:
        raise ValueError(f"convt2x2: in / out channels ({cin}, {cout}) must be multiples of {al} for {dtype} "
                         f"(16-byte pieces of the MFMA GEMM operands)")


def convt2x2_pack(weight: Tensor, dtype: torch.dtype) -> tuple[Tensor, Tensor]:
    """nn.ConvTranspose2d(k=2, s=2) parameter [Cin, Cout, 2, 2] f32 -> (forward operand [4, Cout, Cin] phase-major, data-gradient
    operand [Cin, 4 * Cout]) in ``dtype``, one launch."""
    _need_cuda(weight)
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (2, 2) or weight.dtype != torch.float32 or not weight.is_contiguous():
        raise ValueError(f"convt2x2_pack: contiguous f32 [Cin, Cout, 2, 2] parameter expected, got {tuple(weight.shape)} {weight.dtype}")
    cin, cout = weight.shape[0], weight.shape[1]
    _convt_channels(cin, cout, dtype)
    fwd = torch.empty((4, cout, cin), device=weight.device, dtype=dtype)
    dgrad = torch.empty((cin, 4 * cout), device=weight.device, dtype=dtype)
    _lib.checked().gdl_convt2x2_pack(_p(weight), cin, cout, dt(dtype), _p(fwd), _p(dgrad), _stream())
    return fwd, dgrad


def convt2x2(x: Tensor, w_fwd: Tensor, bias: Tensor | None = None) -> Tensor:
    """F.conv_transpose2d(x, w, bias, stride=2) for a 2x2 kernel on NHWC x [B,H,W,Cin] -> [B,2H,2W,Cout]: the four output phases
    are one batched 1x1 GEMM launch writing the strided phase positions; w_fwd from convt2x2_pack."""
    _need_cuda(x, w_fwd)
    x4 = _nhwc4(x, "convt2x2 x")
    B, H, W, Cc = x4.shape
    if w_fwd.dim() != 3 or w_fwd.shape[0] != 4 or w_fwd.shape[2] != Cc or w_fwd.dtype != x.dtype or not w_fwd.is_contiguous():
        raise ValueError(f"convt2x2: operand must be contiguous [4, Cout, {Cc}] {x.dtype}, got {tuple(w_fwd.shape)} {w_fwd.dtype}")
    N = w_fwd.shape[1]
    _convt_channels(Cc, N, x.dtype)
    y = torch.empty((B, 2 * H, 2 * W, N), device=x.device, dtype=x.dtype)
    a = ConvArgs()
    a.inp, a.dtype = x4.data_ptr(), dt(x4)
    a.B, a.H, a.W, a.C = B, H, W, Cc
    a.in_sB, a.in_sH, a.in_sW = x4.stride(0), x4.stride(1), x4.stride(2)
    a.Ho, a.Wo, a.R, a.S, a.stride, a.pad = H, W, 1, 1, 1, 0
    a.w, a.w_sN, a.N = w_fwd.data_ptr(), Cc, N
    a.out, a.out_dtype = y.data_ptr(), dt(y)
    a.out_sB, a.out_sH, a.out_sW = y.stride(0), 2 * y.stride(1), 2 * y.stride(2)
    a.alpha, a.act = 1.0, ACT_NONE
    a.bias = None if bias is None else _f32vec(bias, N, "bias").data_ptr()
    a.nz, a.nz_inner = 4, 2                                   # z = (row phase, column phase)
    a.w_sZ0, a.w_sZ1 = 2 * N * Cc, N * Cc
    a.out_sZ0, a.out_sZ1 = y.stride(1), y.stride(2)
    batched_gemm_raw(a)
    return y


def convt2x2_dgrad(dy: Tensor, w_dgrad: Tensor) -> Tensor:
    """Data gradient of convt2x2: a 2x2 / stride-2 convolution of dy [B,2H,2W,Cout] with w_dgrad [Cin, 4 * Cout] -> [B,H,W,Cin]."""
    if dy.dim() != 4 or dy.shape[1] % 2 or dy.shape[2] % 2:
        raise ValueError(f"convt2x2_dgrad: dy must be [B, 2H, 2W, Cout], got {tuple(dy.shape)}")
    _convt_channels(w_dgrad.shape[0], dy.shape[3], dy.dtype)
    return conv_gemm(dy, w_dgrad, R=2, S=2, stride=2, pad=0)


def convt2x2_wgrad(x: Tensor, dy: Tensor, out: Tensor | None = None, accumulate: bool = False) -> Tensor:
    """Weight gradient of convt2x2 in the parameter's own layout [Cin, Cout, 2, 2] f32: the weight-gradient GEMM with the roles
    swapped (in = dy under a 2x2 / stride-2 window, dy = x) gives [Cin, (py, px, n)], one kernel re-orders (and, with
    ``accumulate``, adds into ``out``)."""
    _need_cuda(x, dy)
    cin, cout = x.shape[-1], dy.shape[-1]
    _convt_channels(cin, cout, x.dtype)
    if dy.dim() != 4 or x.dim() != 4 or dy.shape[1] != 2 * x.shape[1] or dy.shape[2] != 2 * x.shape[2] or dy.shape[0] != x.shape[0]:
        raise ValueError(f"convt2x2_wgrad: x {tuple(x.shape)} and dy {tuple(dy.shape)} do not belong to one layer")
    dw = conv_wgrad(dy, x, R=2, S=2, stride=2, pad=0)         # [Cin, 4 * Cout]
    if out is None:
        out, accumulate = torch.empty((cin, cout, 2, 2), device=x.device, dtype=torch.float32), False
    elif tuple(out.shape) != (cin, cout, 2, 2) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("convt2x2_wgrad: out must be a contiguous f32 [Cin, Cout, 2, 2] tensor")
    _lib.checked().gdl_convt2x2_unpack_grad(_p(dw), cin, cout, _p(out), int(accumulate), _stream())
    return out


# ------------------------------------------------------------------ resampling
def bilinear(x: Tensor, size: tuple[int, int], out: Tensor | None = None,
             out_dtype: torch.dtype | None = None, accumulate: bool = False) -> Tensor:
    _need_cuda(x)
    x4 = _nhwc4(x, "bilinear x")
    B, Hi, Wi, Cc = x4.shape
    Ho, Wo = size
    if out is None:
        if accumulate:
            raise ValueError("bilinear: accumulate needs out")
        out = torch.empty((B, Ho, Wo, Cc), device=x.device, dtype=out_dtype or x.dtype)
    o4 = _nhwc4(out, "bilinear out")
    if tuple(o4.shape) != (B, Ho, Wo, Cc):
        raise ValueError(f"bilinear: out shape {tuple(o4.shape)} != {(B, Ho, Wo, Cc)}")
    _lib.checked().gdl_bilinear_fwd(_p(x4), dt(x4), B, Hi, Wi, Cc, x4.stride(0), x4.stride(1),
                                    x4.stride(2), _p(o4), dt(o4), Ho, Wo, o4.stride(0),
                                    o4.stride(1), o4.stride(2), int(accumulate), _stream())
    return out


def bilinear_add(base: Tensor, x: Tensor) -> Tensor:
    """base + bilinear(x -> base's size) as a new tensor, in one pass where the fused kernel applies (gdl_bilinear_fwd_add;
    otherwise copy + accumulate inside the library): UperNet's top-down add (upernet.py:127-135)."""
    _need_cuda(base, x)
    b4, x4 = _nhwc4(base, "bilinear_add base"), _nhwc4(x, "bilinear_add x")
    B, Ho, Wo, Cc = b4.shape
    if x4.shape[0] != B or x4.shape[3] != Cc or x4.dtype != b4.dtype:
        raise ValueError(f"bilinear_add: {tuple(x4.shape)} {x4.dtype} does not resize onto {tuple(b4.shape)} {b4.dtype}")
    b4 = b4 if b4.is_contiguous() else b4.contiguous()
    out = torch.empty((B, Ho, Wo, Cc), device=base.device, dtype=base.dtype)
    _lib.checked().gdl_bilinear_fwd_add(_p(x4), dt(x4), B, x4.shape[1], x4.shape[2], Cc, x4.stride(0), x4.stride(1), x4.stride(2),
                                        _p(b4), _p(out), dt(out), Ho, Wo, out.stride(0), out.stride(1), out.stride(2), _stream())
    return out


def bilinear_add_bn(x_pre: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, beta: Tensor, eps: float, relu: bool, x: Tensor) -> Tensor:
    """bilinear_add(bn_apply(x_pre, ...), x) without the normalised map: the top-down add of a training lateral from its
    pre-BatchNorm convolution output ``x_pre``, bit-identical to the two separate ops (gdl_bilinear_fwd_add_bn: dense bf16 maps,
    resize factor 2 or 4; other shapes raise)."""
    _need_cuda(x_pre, x)
    b4, x4 = _nhwc4(x_pre, "bilinear_add_bn base"), _nhwc4(x, "bilinear_add_bn x")
    B, Ho, Wo, Cc = b4.shape
    if x4.shape[0] != B or x4.shape[3] != Cc or x4.dtype != b4.dtype or not b4.is_contiguous() or not x4.is_contiguous():
        raise ValueError(f"bilinear_add_bn: dense maps of one dtype expected, {tuple(x4.shape)} {x4.dtype} onto {tuple(b4.shape)} {b4.dtype}")
    out = torch.empty((B, Ho, Wo, Cc), device=x_pre.device, dtype=x_pre.dtype)
    _lib.checked().gdl_bilinear_fwd_add_bn(_p(x4), dt(x4), B, x4.shape[1], x4.shape[2], Cc, _p(b4), _p(_f32vec(mean, Cc, "mean")),
                                           _p(_f32vec(var, Cc, "var")), _p(_f32vec(gamma, Cc, "gamma")), _p(_f32vec(beta, Cc, "beta")),
                                           eps, int(relu), _p(out), Ho, Wo, _stream())
    return out


GATHER_TWO_PASS = True    # A/B switch (tools / tests): separable two-pass gather for large resize factors


def resize_conv3x3_bwd_gather(dy: Tensor, in_size: tuple[int, int]) -> Tensor:
    """The nine low-resolution maps G_t = resize^T(shift_t^T(dy)) of conv3x3(pad 1)(bilinear resize(x)) as one dense
    [B, Hi, Wi, 9 * N] tensor, tap block 8 - t (see gdl_resize_conv3x3_bwd_gather)."""
    _need_cuda(dy)
    d4 = _nhwc4(dy, "resize_conv3x3_bwd_gather dy")
    if not d4.is_contiguous():
        raise ValueError("resize_conv3x3_bwd_gather: dy must be dense NHWC")
    B, Ho, Wo, N = d4.shape
    Hi, Wi = in_size
    g = torch.empty((B, Hi, Wi, 9 * N), device=dy.device, dtype=dy.dtype)
    lib = _lib.checked()
    one_pass = lib.gdl_resize_conv3x3_bwd_gather_one_pass(dt(d4), B, Ho, Wo, N, Hi, Wi)     # matrix-core form (bf16, x2 / x4)
    if GATHER_TWO_PASS and Ho >= 2 * Hi and not one_pass:      # upsampling factors >= 2: the single VALU pass is multiply-add bound
        nbytes = lib.gdl_resize_conv3x3_bwd_gather_workspace(dt(d4), B, Wo, N, Hi)
        ws = torch.empty(nbytes // d4.element_size(), device=dy.device, dtype=dy.dtype)
        lib.gdl_resize_conv3x3_bwd_gather2(_p(d4), dt(d4), B, Ho, Wo, N, _p(g), Hi, Wi, _p(ws), nbytes, _stream())
    else:
        lib.gdl_resize_conv3x3_bwd_gather(_p(d4), dt(d4), B, Ho, Wo, N, _p(g), Hi, Wi, _stream())
    return g


def resize_conv3x3_bwd_gather_bn_ok(dz: Tensor, in_size: tuple[int, int]) -> bool:
    """Shapes the BatchNorm-backward-fused gather takes (= the one-pass matrix-core gather: bf16, N % 64 == 0, factor 2 / 4)."""
    if dz.dim() != 4 or dz.dtype != torch.bfloat16 or not dz.is_contiguous():
        return False
    B, Ho, Wo, N = dz.shape
    return bool(_lib.load().gdl_resize_conv3x3_bwd_gather_one_pass(dt(dz), B, Ho, Wo, N, in_size[0], in_size[1]))


def resize_conv3x3_bwd_gather_bn(dz: Tensor, y: Tensor, in_size: tuple[int, int], mean, var, gamma, beta, eps, relu, dgamma_sum,
                                 dbeta_sum, p_total) -> Tensor:
    """resize_conv3x3_bwd_gather(bn_bwd_dx(y, dz, ...)) in one kernel: the BatchNorm(+ReLU) backward is applied to dz while it is
    staged, its result is never written (gdl_resize_conv3x3_bwd_gather_bn).  dz, y dense NHWC bf16 of one shape."""
    _need_cuda(dz, y)
    if dz.shape != y.shape or dz.dtype != y.dtype or not (dz.is_contiguous() and y.is_contiguous()):
        raise ValueError("resize_conv3x3_bwd_gather_bn: dz and y must be dense NHWC tensors of one shape and dtype")
    B, Ho, Wo, N = dz.shape
    Hi, Wi = in_size
    g = torch.empty((B, Hi, Wi, 9 * N), device=dz.device, dtype=dz.dtype)
    coef = torch.empty(4 * N, device=dz.device, dtype=torch.float32)
    _lib.checked().gdl_resize_conv3x3_bwd_gather_bn(_p(dz), _p(y), dt(dz), B, Ho, Wo, N, _p(g), Hi, Wi, _p(mean), _p(var), _p(gamma),
                                                    _p(beta), eps, int(relu), _p(dgamma_sum), _p(dbeta_sum), p_total, _p(coef),
                                                    _stream())
    return g


def resize_conv3x3_bwd(x_lo: Tensor, dy: Tensor | None, w_dgrad: Tensor | None, want_dw: bool = True, g: Tensor | None = None):
    """(dx_lo, dw) of y = conv3x3(pad 1)(bilinear resize(x_lo -> dy's size)) from dy, as GEMMs over the LOW-resolution
    pixels.  ``w_dgrad`` [C, 9 * N] (gdl_pack_dgrad operand; None = no data gradient); dw [N, 9 * C] f32.  ``g``: the nine
    gathered maps when the caller already has them (resize_conv3x3_bwd_gather_bn), dy is then unused."""
    x4 = _nhwc4(x_lo, "resize_conv3x3_bwd x")
    B, Hi, Wi, Cc = x4.shape
    if g is None:
        g = resize_conv3x3_bwd_gather(dy, (Hi, Wi))
    N = g.shape[-1] // 9
    dx = conv_gemm(g, w_dgrad) if w_dgrad is not None else None
    dw = None
    if want_dw:
        # one 1x1 weight gradient with the nine maps as 9 N "output channels": [(8 - t, n), c] -> [n, (t, c)]
        dwp = conv_wgrad(x4, g, R=1, S=1)
        dw = dwp.view(9, N, Cc).flip(0).permute(1, 0, 2).reshape(N, 9 * Cc)
    return dx, dw


def resize_conv3x3_fwd_sum(zs: list[Tensor], size: tuple[int, int], addvec: Tensor | None = None, relu: bool = False) -> Tensor:
    """sum_k sum_t shift_t(bilinear(zs[k][..., t*N:(t+1)*N] -> size)) (+ addvec, ReLU): the pixel side of
    conv3x3(pad 1)(bilinear resize(x)) once the nine tap products z = [W_0 x, ..., W_8 x] exist at low resolution
    (gdl_resize_conv3x3_fwd_sum).  zs: 1..3 dense [B, h_k, w_k, 9 N] maps of one dtype.  Sources whose size divides ``size`` by
    2 / 4 / 8 go through the cell kernels (matrix cores in bf16) in ONE pass; any other ratio (DOFA-large's 36 -> 292) is added
    by the plain gather kernel, one pass per such source (gdl_resize_conv3x3_fwd_sum_any)."""
    _need_cuda(*zs)
    if not 1 <= len(zs) <= 3:
        raise ValueError("resize_conv3x3_fwd_sum: 1..3 sources")
    z4 = [_nhwc4(z, "resize_conv3x3_fwd_sum source") for z in zs]
    B, N9 = z4[0].shape[0], z4[0].shape[3]
    if N9 % 9:
        raise ValueError("resize_conv3x3_fwd_sum: sources must have 9 * N channels")
    N = N9 // 9
    for z in z4:
        if z.shape[0] != B or z.shape[3] != N9 or z.dtype != z4[0].dtype or not z.is_contiguous():
            raise ValueError("resize_conv3x3_fwd_sum: sources must be contiguous NHWC maps with equal batch, channels and dtype")
    out = torch.empty((B, size[0], size[1], N), device=zs[0].device, dtype=zs[0].dtype)
    cell = [z for z in z4 if resize_conv3x3_fwd_ok((z.shape[1], z.shape[2]), size, B)]
    other = [z for z in z4 if not resize_conv3x3_fwd_ok((z.shape[1], z.shape[2]), size, B)]
    lib = _lib.checked()
    av = _f32vec(addvec, N, "addvec")
    if cell:
        n = len(cell)
        ptrs = (C.c_void_p * 3)(*([z.data_ptr() for z in cell] + [None] * (3 - n)))
        hs = (C.c_int * 3)(*([z.shape[1] for z in cell] + [1] * (3 - n)))
        ws = (C.c_int * 3)(*([z.shape[2] for z in cell] + [1] * (3 - n)))
        # (addvec and the ReLU belong to the LAST pass over `out`)
        lib.gdl_resize_conv3x3_fwd_sum(ptrs, hs, ws, n, dt(cell[0]), B, N, _p(out), size[0], size[1],
                                       _p(None if other else av), int(relu and not other), _stream())
    for i, z in enumerate(other):
        last = i == len(other) - 1
        lib.gdl_resize_conv3x3_fwd_sum_any(_p(z), z.shape[1], z.shape[2], dt(z), B, N, _p(out), size[0], size[1],
                                           int(bool(cell) or i > 0), _p(av if last else None), int(relu and last), _stream())
    return out


def resize_conv3x3_fwd_sum_bn(zs: list[Tensor], size: tuple[int, int], addvec: Tensor | None = None,
                              running_mean: Tensor | None = None, running_var: Tensor | None = None, momentum: float = 0.1):
    """resize_conv3x3_fwd_sum + the train-mode BatchNorm statistics of its result in the same pass
    (gdl_resize_conv3x3_fwd_sum_bn): returns (out, mean, biased var); updates the running buffers when given.  bf16, N % 64 == 0."""
    _need_cuda(*zs)
    z4 = [_nhwc4(z, "resize_conv3x3_fwd_sum_bn source") for z in zs]
    B, N9 = z4[0].shape[0], z4[0].shape[3]
    N = N9 // 9
    for z in z4:
        if z.shape[0] != B or z.shape[3] != N9 or z.dtype != z4[0].dtype or not z.is_contiguous():
            raise ValueError("resize_conv3x3_fwd_sum_bn: sources must be contiguous NHWC maps with equal batch, channels and dtype")
    out = torch.empty((B, size[0], size[1], N), device=zs[0].device, dtype=zs[0].dtype)
    mean = torch.empty(N, device=out.device, dtype=torch.float32)
    var = torch.empty_like(mean)
    lib = _lib.checked()
    rows = lib.gdl_resize_conv3x3_fwd_sum_bn_rows(B, size[0], size[1])
    wsp = torch.empty(rows * 2 * N, device=out.device, dtype=torch.float32)
    n = len(z4)
    ptrs = (C.c_void_p * 3)(*([z.data_ptr() for z in z4] + [None] * (3 - n)))
    hs = (C.c_int * 3)(*([z.shape[1] for z in z4] + [1] * (3 - n)))
    ws = (C.c_int * 3)(*([z.shape[2] for z in z4] + [1] * (3 - n)))
    lib.gdl_resize_conv3x3_fwd_sum_bn(ptrs, hs, ws, n, dt(z4[0]), B, N, _p(out), size[0], size[1],
                                      _p(_f32vec(addvec, N, "addvec")), _p(wsp), wsp.numel() * 4, _p(mean), _p(var),
                                      _p(running_mean), _p(running_var), momentum, _stream())
    return out, mean, var


def resize_conv3x3_fwd_bn_ok(z_dtype: torch.dtype, N: int, addvec: Tensor | None = None) -> bool:
    """The statistics variant runs on the matrix-core kernel only: bf16, N % 64 == 0 and a per-channel addend (bias) the
    kernel can fetch with 16-byte loads (a bias that is a view at an odd offset falls back to the separate statistics pass)."""
    if addvec is not None and addvec.data_ptr() % 16:
        return False
    return z_dtype == torch.bfloat16 and N % 64 == 0


def resize_conv3x3_fwd_ok(lo: tuple[int, int], size: tuple[int, int], B: int) -> bool:
    """Shapes gdl_resize_conv3x3_fwd_sum takes: one integer factor of 2, 4 or 8 in both directions, B * rows in one grid dim."""
    f = size[0] // max(lo[0], 1)
    return f in (2, 4, 8) and lo[0] * f == size[0] and lo[1] * f == size[1] and B * size[0] <= 65535


MAX_ANY_RESIZE = 10.0     # the backward gather's widest window instantiation (2 * ceil(factor) + 4 <= 24 columns)


def resize_conv3x3_any_ok(lo: tuple[int, int], size: tuple[int, int], B: int) -> bool:
    """Upsampling ratios the low-resolution forms of conv3x3(resize(x)) take at all: any real factor in (1, 10] per direction
    (forward: resize_conv3x3_fwd_sum's plain gather pass; backward: the gather kernels' window instantiations)."""
    fy, fx = size[0] / max(lo[0], 1), size[1] / max(lo[1], 1)
    return 1.0 < fy <= MAX_ANY_RESIZE and 1.0 < fx <= MAX_ANY_RESIZE and B * size[0] <= 65535


def copy_cast(x: Tensor, out: Tensor | None = None, out_dtype: torch.dtype | None = None) -> Tensor:
    """Strided NHWC copy with dtype conversion (f32 / bf16): dense copy of a channel slice, compute-dtype cast."""
    _need_cuda(x)
    x4 = _nhwc4(x, "copy_cast x")
    B, H, W, Cc = x4.shape
    if out is None:
        out = torch.empty(x4.shape, device=x.device, dtype=out_dtype or x.dtype)
    o4 = _nhwc4(out, "copy_cast out")
    if tuple(o4.shape) != (B, H, W, Cc):
        raise ValueError(f"copy_cast: out shape {tuple(o4.shape)} != {(B, H, W, Cc)}")
    if B * H > 65535 or Cc % 4:        # very tall batches / odd channel counts: the identity resample handles any layout
        return bilinear(x, (H, W), out=out)      # (same HBM-bound copy through the flat-index kernel: no slow path to warn about)
    _lib.checked().gdl_copy_cast(_p(x4), dt(x4), B, H, W, Cc, x4.stride(0), x4.stride(1), x4.stride(2), _p(o4), dt(o4),
                                 o4.stride(0), o4.stride(1), o4.stride(2), _stream())
    return out


def bilinear_sum(xs: list[Tensor], size: tuple[int, int]) -> Tensor:
    """sum_k bilinear(xs[k] -> size) for 1..3 dense NHWC maps with equal batch / channels / dtype, one output write."""
    _need_cuda(*xs)
    if not 1 <= len(xs) <= 3:
        raise ValueError("bilinear_sum: 1..3 sources")
    x4s = [_nhwc4(x, "bilinear_sum source") for x in xs]
    B, _, _, Cc = x4s[0].shape
    for x in x4s:
        if x.shape[0] != B or x.shape[3] != Cc or x.dtype != x4s[0].dtype or not x.is_contiguous():
            raise ValueError("bilinear_sum: sources must be contiguous NHWC maps with equal batch, channels and dtype")
    out = torch.empty((B, size[0], size[1], Cc), device=xs[0].device, dtype=xs[0].dtype)
    n = len(x4s)
    ptrs = (C.c_void_p * 3)(*([x.data_ptr() for x in x4s] + [None] * (3 - n)))
    hs = (C.c_int * 3)(*([x.shape[1] for x in x4s] + [1] * (3 - n)))
    ws = (C.c_int * 3)(*([x.shape[2] for x in x4s] + [1] * (3 - n)))
    _lib.checked().gdl_bilinear_sum_fwd(ptrs, hs, ws, n, dt(x4s[0]), B, Cc, _p(out), size[0], size[1], _stream())
    return out


def bilinear_bwd(dout: Tensor, in_size: tuple[int, int], din: Tensor | None = None,
                 din_dtype: torch.dtype | None = None, accumulate: bool = False) -> Tensor:
    d4 = _nhwc4(dout, "bilinear_bwd dout")
    B, Ho, Wo, Cc = d4.shape
    Hi, Wi = in_size
    if din is None:
        din = torch.empty((B, Hi, Wi, Cc), device=dout.device, dtype=din_dtype or dout.dtype)
    i4 = _nhwc4(din, "bilinear_bwd din")
    _lib.checked().gdl_bilinear_bwd(_p(d4), dt(d4), B, Ho, Wo, Cc, d4.stride(0), d4.stride(1),
                                    d4.stride(2), _p(i4), dt(i4), Hi, Wi, i4.stride(0),
                                    i4.stride(1), i4.stride(2), int(accumulate), _stream())
    return din


def adaptive_avgpool(x: Tensor, s: int, out_dtype: torch.dtype | None = None) -> Tensor:
    x4 = _nhwc4(x, "avgpool x")
    B, Hi, Wi, Cc = x4.shape
    out = torch.empty((B, s, s, Cc), device=x.device, dtype=out_dtype or x.dtype)
    _lib.checked().gdl_adaptive_avgpool_fwd(_p(x4), dt(x4), B, Hi, Wi, Cc, x4.stride(0),
                                            x4.stride(1), x4.stride(2), _p(out), dt(out), s,
                                            _stream())
    return out


def adaptive_avgpool_bwd(dout: Tensor, in_size: tuple[int, int], din: Tensor | None = None,
                         accumulate: bool = False) -> Tensor:
    if not dout.is_contiguous():
        raise ValueError("adaptive_avgpool_bwd: dout must be contiguous NHWC")
    B, s, _, Cc = dout.shape
    Hi, Wi = in_size
    if din is None:
        din = torch.empty((B, Hi, Wi, Cc), device=dout.device, dtype=dout.dtype)
    i4 = _nhwc4(din, "avgpool_bwd din")
    _lib.checked().gdl_adaptive_avgpool_bwd(_p(dout), dt(dout), B, s, Cc, _p(i4), dt(i4), Hi, Wi,
                                            i4.stride(0), i4.stride(1), i4.stride(2),
                                            int(accumulate), _stream())
    return din


# ------------------------------------------------------------------ fused bilinear x4 upsample -> 3x3 conv
def pad_nhwc(x: Tensor, pad_h: int, pad_w: int, zero: bool = False) -> Tensor:
    """NHWC border padding: replicate (default) or zeros."""
    _need_cuda(x)
    x4 = _nhwc4(x, "pad_nhwc x")
    B, H, W, Cc = x4.shape
    out = torch.empty((B, H + 2 * pad_h, W + 2 * pad_w, Cc), device=x.device, dtype=x.dtype)
    _lib.checked().gdl_pad_nhwc(_p(x4), dt(x4), B, H, W, Cc, x4.stride(0), x4.stride(1), x4.stride(2), _p(out),
                                pad_h, pad_w, int(zero), _stream())
    return out


def subpix4_weights(w32: Tensor, Cc: int, out_dtype: torch.dtype) -> dict:
    """Phase weights of (bilinear x4 upsample -> 3x3 conv) from w32 [N, 9*C] f32 (K order dy,dx,c); csrc/subpixel.hip."""
    _need_cuda(w32)
    N = w32.shape[0]
    if w32.dtype != torch.float32 or not w32.is_contiguous() or w32.shape[1] != 9 * Cc:
        raise ValueError("subpix4_weights: contiguous f32 [N, 9*C] expected")
    mk = lambda taps: torch.empty((4, N, taps * Cc), device=w32.device, dtype=out_dtype)  # noqa: E731
    out = {"g22": mk(4), "g23": mk(6), "g32": mk(6), "g33": mk(9), "lines": mk(3)}
    _lib.checked().gdl_subpix4_weights(_p(w32), N, Cc, dt(out["g22"]), _p(out["g22"]), _p(out["g23"]), _p(out["g32"]),
                                       _p(out["g33"]), _p(out["lines"]), _stream())
    return out


def up4_conv3x3(x: Tensor, wsets: dict, *, bias: Tensor | None = None, scale: Tensor | None = None,
                shift: Tensor | None = None, act: int = ACT_NONE) -> Tensor:
    """conv3x3(pad 1)(bilinear_x4(x)) on NHWC x [B,H,W,C] WITHOUT materialising the upsampled map: 16 phase
    convolutions of the replicate-padded low-res map (four batched launches, 6.25 low-res taps on average instead of 9
    high-res ones) written into the strided phase positions of the output, then the four outermost output lines --
    the only ones the convolution's zero padding touches -- recomputed exactly by 1x3 line convolutions.
    Reference: multilevel_neck.py:157-158 with scale 4 (+ models/utils.py:131-137)."""
    _need_cuda(x)
    x4 = _nhwc4(x, "up4_conv3x3 x")
    B, H, W, Cc = x4.shape
    N = wsets["g22"].shape[1]
    es = x4.element_size()
    xp = pad_nhwc(x4, 1, 1)                                   # replicate: the bilinear index clamping
    Hp, Wp = H + 2, W + 2
    y = torch.empty((B, 4 * H, 4 * W, N), device=x.device, dtype=x.dtype)
    f32 = lambda t, name: None if t is None else _f32vec(t, N, name).data_ptr()  # noqa: E731
    for gy, R in ((0, 2), (1, 3)):
        for gx, S in ((0, 2), (1, 3)):
            wg = wsets[f"g{R}{S}"]
            py0, dpy = (0, 3) if R == 2 else (1, 1)
            px0, dpx = (0, 3) if S == 2 else (1, 1)
            a = ConvArgs()
            a.inp, a.dtype = xp.data_ptr(), dt(xp)
            a.B, a.H, a.W, a.C = B, H + R - 1, W + S - 1, Cc
            a.in_sB, a.in_sH, a.in_sW = Hp * Wp * Cc, Wp * Cc, Cc
            a.Ho, a.Wo, a.R, a.S, a.stride, a.pad = H, W, R, S, 1, 0
            a.w, a.w_sN, a.N = wg.data_ptr(), R * S * Cc, N
            a.out = y.data_ptr() + (py0 * 4 * W * N + px0 * N) * es
            a.out_dtype = dt(y)
            a.out_sB, a.out_sH, a.out_sW = 16 * H * W * N, 16 * W * N, 4 * N
            a.alpha, a.act = 1.0, act
            a.bias, a.scale, a.shift = f32(bias, "bias"), f32(scale, "scale"), f32(shift, "shift")
            a.nz, a.nz_inner = 4, 2                           # z = (row phase index, column phase index)
            a.in_sZ0, a.in_sZ1 = (Wp * Cc if R == 2 else 0), (Cc if S == 2 else 0)
            a.w_sZ0, a.w_sZ1 = 2 * N * R * S * Cc, N * R * S * Cc
            a.out_sZ0, a.out_sZ1 = dpy * 4 * W * N, dpx * N
            batched_gemm_raw(a)
    lines = wsets["lines"]
    for side, (ln, view) in enumerate(zip(_up4_lines(x4), _up4_line_views(y))):
        conv_gemm(ln, lines[side], R=1, S=3, out=view, bias=bias, scale=scale, shift=shift, act=act)
    return y


def _up4_lines(x4: Tensor):
    """The four zero-extended border lines of the x4-upsampled map (top, bottom, left, right), each [B,1,4L+2,C]."""
    B, H, W, Cc = x4.shape
    out = []
    for src in (x4[:, 0:1], x4[:, H - 1:H]):
        out.append(pad_nhwc(bilinear(src, (1, 4 * W)), 0, 1, zero=True))
    for src in (x4[:, :, 0:1], x4[:, :, W - 1:W]):
        out.append(pad_nhwc(bilinear(src, (4 * H, 1)).view(B, 1, 4 * H, Cc), 0, 1, zero=True))
    return out


def _up4_line_views(y: Tensor):
    """The matching output lines of y [B,4H,4W,N] as [B,1,L,N] views."""
    Hh, Ww = y.shape[1], y.shape[2]
    return [y[:, 0:1], y[:, Hh - 1:Hh], y[:, :, 0, :].unsqueeze(1), y[:, :, Ww - 1, :].unsqueeze(1)]


# ------------------------------------------------------------------ attention (unfused + fused)
def _attn_check(q: Tensor, k: Tensor, v: Tensor, num_heads: int):
    _need_cuda(q, k, v)
    if q.dim() != 3 or k.dim() != 3 or v.shape != k.shape or q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2]:
        raise ValueError("attention: expected q [B,Nq,D], k/v [B,Nkv,D]")
    if not (q.dtype == k.dtype == v.dtype) or q.stride(2) != 1 or k.stride(2) != 1 or v.stride(2) != 1:
        raise ValueError("attention: q/k/v must share a dtype and have unit channel stride")
    B, Nq, D = q.shape
    return B, Nq, k.shape[1], D, D // num_heads


def _v_transposed(v: Tensor, num_heads: int, hd: int, npad: int) -> Tensor:
    B, Nkv, _ = v.shape
    vt = torch.empty((B, num_heads, hd, npad), device=v.device, dtype=v.dtype)
    _lib.checked().gdl_v_transpose(_p(v), dt(v), B, Nkv, num_heads, hd, v.stride(0), v.stride(1), _p(vt),
                                   npad, _stream())
    return vt


def attention_unfused(q: Tensor, k: Tensor, v: Tensor, num_heads: int) -> Tensor:
    """softmax(q k^T / sqrt(hd)) v with materialised scores: the exact-f32 parity path (and the
    small / odd-head-dim cases).  q [B,Nq,D], k,v [B,Nkv,D] (strided views allowed, e.g. slices of
    a packed qkv or kv tensor).  Returns [B,Nq,D]."""
    B, Nq, Nkv, D, hd = _attn_check(q, k, v, num_heads)
    es = 4 if q.dtype == torch.float32 else 2
    al = 16 // es
    if hd % al != 0:
        raise ValueError(f"attention: head_dim {hd} must be a multiple of {al} for {q.dtype}")
    npad = (Nkv + 63) // 64 * 64
    lib = _lib.checked()
    vt = _v_transposed(v, num_heads, hd, npad)
    scores = torch.empty((B, num_heads, Nq, npad), device=q.device, dtype=q.dtype)
    a = ConvArgs()
    a.inp, a.dtype = q.data_ptr(), dt(q)
    a.B, a.H, a.W, a.C = 1, 1, Nq, hd
    a.in_sB, a.in_sH, a.in_sW = Nq * q.stride(1), Nq * q.stride(1), q.stride(1)
    a.Ho, a.Wo, a.R, a.S, a.stride, a.pad = 1, Nq, 1, 1, 1, 0
    a.w, a.w_sN, a.N = k.data_ptr(), k.stride(1), Nkv
    a.out, a.out_dtype = scores.data_ptr(), dt(scores)
    a.out_sB, a.out_sH, a.out_sW = Nq * npad, Nq * npad, npad
    a.alpha, a.act = float(hd) ** -0.5, ACT_NONE
    a.nz, a.nz_inner = B * num_heads, num_heads
    a.in_sZ0, a.in_sZ1 = q.stride(0), hd
    a.w_sZ0, a.w_sZ1 = k.stride(0), hd
    a.out_sZ0, a.out_sZ1 = num_heads * Nq * npad, Nq * npad
    batched_gemm_raw(a)
    lib.gdl_softmax_rows(_p(scores), _p(scores), dt(scores), B * num_heads * Nq, Nkv, npad,
                         _stream())
    out = torch.empty((B, Nq, D), device=q.device, dtype=q.dtype)
    a = ConvArgs()
    a.inp, a.dtype = scores.data_ptr(), dt(scores)
    a.B, a.H, a.W, a.C = 1, 1, Nq, npad
    a.in_sB, a.in_sH, a.in_sW = Nq * npad, Nq * npad, npad
    a.Ho, a.Wo, a.R, a.S, a.stride, a.pad = 1, Nq, 1, 1, 1, 0
    a.w, a.w_sN, a.N = vt.data_ptr(), npad, hd
    a.out, a.out_dtype = out.data_ptr(), dt(out)
    a.out_sB, a.out_sH, a.out_sW = Nq * D, Nq * D, D
    a.alpha, a.act = 1.0, ACT_NONE
    a.nz, a.nz_inner = B * num_heads, num_heads
    a.in_sZ0, a.in_sZ1 = num_heads * Nq * npad, Nq * npad
    a.w_sZ0, a.w_sZ1 = num_heads * hd * npad, hd * npad
    a.out_sZ0, a.out_sZ1 = Nq * D, hd
    batched_gemm_raw(a)
    return out


def attention_flash(q: Tensor, k: Tensor, v: Tensor, num_heads: int, return_lse: bool = False):
    """Fused flash attention forward (bf16, head_dim 64); same argument convention.  V is read row-major (transposed
    inside the LDS).  ``return_lse``: also return the log-sum-exp of the scaled scores [B,H,Nq] f32, which the fused
    backward recomputes the probabilities from."""
    B, Nq, Nkv, D, hd = _attn_check(q, k, v, num_heads)
    if q.dtype != torch.bfloat16 or hd != 64:
        raise ValueError("attention_flash: needs bf16 and head_dim 64")
    out = torch.empty((B, Nq, D), device=q.device, dtype=q.dtype)
    lse = torch.empty((B, num_heads, Nq), device=q.device, dtype=torch.float32) if return_lse else None
    _lib.checked().gdl_flash_attn_fwd2(_p(q), q.stride(0), q.stride(1), _p(k), k.stride(0), k.stride(1),
                                       _p(v), v.stride(0), v.stride(1), _p(out), out.stride(0), out.stride(1),
                                       _p(lse), B, num_heads, Nq, Nkv, float(hd) ** -0.5, _stream())
    return (out, lse) if return_lse else out


def attention_flash_v1(q: Tensor, k: Tensor, v: Tensor, num_heads: int) -> Tensor:
    """First-generation kernel (separate V^T pass); kept for A/B measurements."""
    B, Nq, Nkv, D, hd = _attn_check(q, k, v, num_heads)
    npad = (Nkv + 63) // 64 * 64
    vt = _v_transposed(v, num_heads, hd, npad)
    out = torch.empty((B, Nq, D), device=q.device, dtype=q.dtype)
    _lib.checked().gdl_flash_attn_fwd(_p(q), q.stride(0), q.stride(1), _p(k), k.stride(0), k.stride(1),
                                      _p(vt), _p(out), B, num_heads, Nq, Nkv, npad, float(hd) ** -0.5,
                                      _stream())
    return out


def flash_ok(q: Tensor, num_heads: int) -> bool:
    return q.dtype == torch.bfloat16 and q.shape[2] // num_heads == 64


def attention(q: Tensor, k: Tensor, v: Tensor, num_heads: int, return_lse: bool = False):
    """Dispatch: flash kernel for bf16 / head_dim 64, materialised-score path otherwise (lse = None there)."""
    if flash_ok(q, num_heads):
        return attention_flash(q, k, v, num_heads, return_lse)
    out = attention_unfused(q, k, v, num_heads)
    return (out, None) if return_lse else out


def attention_flash_bwd(q: Tensor, k: Tensor, v: Tensor, o: Tensor, do: Tensor, lse: Tensor, num_heads: int,
                        dq: Tensor, dk: Tensor, dv: Tensor) -> None:
    """Fused attention backward (bf16, head_dim 64): dq / dk / dv written in place (strided slices allowed)."""
    B, Nq, Nkv, D, hd = _attn_check(q, k, v, num_heads)
    for t, n in ((o, Nq), (do, Nq), (dq, Nq), (dk, Nkv), (dv, Nkv)):
        if t.shape != (B, n, D) or t.dtype != torch.bfloat16 or t.stride(2) != 1:
            raise ValueError("attention_flash_bwd: tensor shape / dtype / stride mismatch")
    if lse.shape != (B, num_heads, Nq) or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise ValueError("attention_flash_bwd: lse must be contiguous f32 [B,H,Nq]")
    dvec = torch.empty_like(lse)
    nbytes = _lib.load().gdl_flash_attn_bwd_workspace(B, num_heads, Nq, Nkv)
    ws = torch.empty(nbytes // 4, device=q.device, dtype=torch.float32) if nbytes else None
    _lib.checked().gdl_flash_attn_bwd(
        _p(q), q.stride(0), q.stride(1), _p(k), k.stride(0), k.stride(1), _p(v), v.stride(0), v.stride(1),
        _p(o), o.stride(0), o.stride(1), _p(do), do.stride(0), do.stride(1), _p(lse), _p(dvec),
        _p(dq), dq.stride(0), dq.stride(1), _p(dk), dk.stride(0), dk.stride(1), _p(dv), dv.stride(0), dv.stride(1),
        B, num_heads, Nq, Nkv, float(hd) ** -0.5, _p(ws), nbytes, _stream())


def split_qkv(qkv: Tensor):
    """[B,N,3D] packed timm qkv -> three strided views [B,N,D] (no copy)."""
    D = qkv.shape[-1] // 3
    return qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]


def dwconv3x3(x: Tensor, w9: Tensor, bias: Tensor, gelu: bool, out_dtype: torch.dtype | None = None) -> Tensor:
    """Depthwise 3x3 (pad 1) + bias (+GELU) on a contiguous NHWC tensor; w9 is [9, C] f32."""
    _need_cuda(x)
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("dwconv3x3: contiguous NHWC input expected")
    B, H, W, Cc = x.shape
    if w9.shape != (9, Cc) or w9.dtype != torch.float32 or not w9.is_contiguous():
        raise ValueError("dwconv3x3: w9 must be contiguous f32 [9, C]")
    out = torch.empty(x.shape, device=x.device, dtype=out_dtype or x.dtype)
    _lib.checked().gdl_dwconv3x3(_p(x), dt(x), B, H, W, Cc, _p(w9), _p(_f32vec(bias, Cc, "bias")), int(gelu),
                                 _p(out), dt(out), _stream())
    return out


# ------------------------------------------------------------------ transformer-block backward
def _colreduce_ws(rows: int, Cc: int, planes: int, device) -> tuple[Tensor, int]:
    nbytes = _lib.load().gdl_colreduce_workspace(rows, Cc, planes)
    return torch.empty(max(nbytes, 4) // 4, device=device, dtype=torch.float32), nbytes


def layernorm_bwd(x: Tensor, dy: Tensor, gamma: Tensor, eps: float, dres: Tensor | None = None,
                  dgamma: Tensor | None = None, dbeta: Tensor | None = None, accumulate: bool = False):
    """-> (dx f32 like x, dgamma, dbeta); ``dres`` (f32, x's shape) is added into dx."""
    _need_cuda(x, dy)
    D = x.shape[-1]
    if x.dtype != torch.float32 or x.stride(-1) != 1 or not dy.is_contiguous() or dy.shape != x.shape:
        raise ValueError("layernorm_bwd: x f32 with unit last stride, dy contiguous of the same shape")
    x2 = x.reshape(-1, D)
    rows = x2.shape[0]
    dx = torch.empty((rows, D), device=x.device, dtype=torch.float32)
    r2 = None
    if dres is not None:
        if dres.dtype != torch.float32 or dres.shape != x.shape or dres.stride(-1) != 1:
            raise ValueError("layernorm_bwd: dres must be f32 of x's shape")
        r2 = dres.reshape(-1, D)
    dgamma = torch.empty(D, device=x.device, dtype=torch.float32) if dgamma is None else dgamma
    dbeta = torch.empty(D, device=x.device, dtype=torch.float32) if dbeta is None else dbeta
    ws, nbytes = _colreduce_ws(rows, D, 2, x.device)
    _lib.checked().gdl_layernorm_bwd(_p(x2), x2.stride(0), _p(dy), dt(dy), _p(_f32vec(gamma, D, "gamma")), _p(r2),
                                     0 if r2 is None else r2.stride(0), _p(dx), D, rows, D, eps, _p(dgamma),
                                     _p(dbeta), int(accumulate), _p(ws), nbytes, _stream())
    return dx.reshape(x.shape), dgamma, dbeta


def colsum(x: Tensor, out: Tensor | None = None, accumulate: bool = False) -> Tensor:
    """out[c] (+)= sum over all leading dims of x[..., c] (bias gradients)."""
    _need_cuda(x)
    Cc = x.shape[-1]
    x2 = x.reshape(-1, Cc)
    if x2.stride(1) != 1:
        raise ValueError("colsum: unit channel stride expected")
    if out is None:
        out = torch.empty(Cc, device=x.device, dtype=torch.float32)
    ws, nbytes = _colreduce_ws(x2.shape[0], Cc, 1, x.device)
    _lib.checked().gdl_colsum(_p(x2), dt(x2), x2.shape[0], Cc, x2.stride(0), _p(out), int(accumulate), _p(ws),
                              nbytes, _stream())
    return out


def layerscale_bwd(g: Tensor, z: Tensor | None, gamma: Tensor | None, batch_scale: Tensor | None,
                   out_dtype: torch.dtype, dgamma: Tensor | None = None, accumulate: bool = False):
    """g f32 [B,N,C] -> (dz [B,N,C] in out_dtype = g*batch_scale*gamma, dgamma = sum g*batch_scale*z or None)."""
    _need_cuda(g)
    B, N, Cc = g.shape
    if g.dtype != torch.float32 or not g.is_contiguous():
        raise ValueError("layerscale_bwd: contiguous f32 gradient expected")
    dz = torch.empty((B, N, Cc), device=g.device, dtype=out_dtype)
    ws, nbytes = (None, 0)
    if gamma is not None:
        if z is None or not z.is_contiguous() or z.shape != g.shape:
            raise ValueError("layerscale_bwd: z must be contiguous and of g's shape")
        dgamma = torch.empty(Cc, device=g.device, dtype=torch.float32) if dgamma is None else dgamma
        ws, nbytes = _colreduce_ws(B * N, Cc, 1, g.device)
    zz = z if gamma is not None else None
    _lib.checked().gdl_layerscale_bwd(_p(g), _p(zz), F32 if zz is None else dt(zz),
                                      _p(None if gamma is None else _f32vec(gamma, Cc, "gamma")),
                                      _p(None if batch_scale is None else _f32vec(batch_scale, B, "batch_scale")),
                                      B * N, N, Cc, _p(dz), dt(dz), _p(dgamma if gamma is not None else None),
                                      int(accumulate), _p(ws), nbytes, _stream())
    return dz, (dgamma if gamma is not None else None)


def dwconv3x3_gelu_bwd(u: Tensor, dy: Tensor, w9: Tensor, bias: Tensor):
    """backward of gelu(dwconv3x3(u)+bias): -> (du like u, dw9 [9,C] f32, dbias [C] f32)."""
    _need_cuda(u, dy)
    if u.dim() != 4 or not u.is_contiguous() or not dy.is_contiguous() or dy.shape != u.shape or dy.dtype != u.dtype:
        raise ValueError("dwconv3x3_gelu_bwd: contiguous NHWC u and dy of one dtype expected")
    B, H, W, Cc = u.shape
    dpre = torch.empty_like(u)
    dw9 = torch.empty((9, Cc), device=u.device, dtype=torch.float32)
    db = torch.empty(Cc, device=u.device, dtype=torch.float32)
    ws, nbytes = _colreduce_ws(B * H * W, Cc, 10, u.device)
    _lib.checked().gdl_dwconv3x3_gelu_bwd(_p(u), _p(dy), dt(u), B, H, W, Cc, _p(w9), _p(_f32vec(bias, Cc, "bias")),
                                          _p(dpre), _p(dw9), _p(db), 0, _p(ws), nbytes, _stream())
    zero_b = torch.zeros(Cc, device=u.device, dtype=torch.float32)
    du = dwconv3x3(dpre, w9.flip(0).contiguous(), zero_b, False)
    return du, dw9, db


# ------------------------------------------------------------------ dynamic (channel-adaptive) SegFormer stem
def _f32c(t: Tensor, shape: tuple, name: str) -> Tensor:
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous f32 tensor of shape {tuple(shape)}, got {tuple(t.shape)} {t.dtype}")
    return t


def chan_weights(pos: Tensor, W0: Tensor, b0: Tensor, W2: Tensor, b2: Tensor, W1: Tensor, b1: Tensor):
    """weight_gen + the position half of channel_attention[0] (mix_transformer.py:781-801).
    pos [C, PD]; W1 = channel_attention.0.weight as [H1, E + PD].  -> (hid [C,HD], cw [C,E], hb [C,H1])"""
    _need_cuda(pos, W0, W2, W1)
    Cn, PD = pos.shape
    HD, E, H1 = W0.shape[0], W2.shape[0], W1.shape[0]
    _f32c(pos, (Cn, PD), "pos"), _f32c(W0, (HD, PD), "weight_gen.0.weight"), _f32c(W2, (E, HD), "weight_gen.2.weight")
    _f32c(W1, (H1, E + PD), "channel_attention.0.weight")
    hid = torch.empty((Cn, HD), device=pos.device, dtype=torch.float32)
    cw = torch.empty((Cn, E), device=pos.device, dtype=torch.float32)
    hb = torch.empty((Cn, H1), device=pos.device, dtype=torch.float32)
    w1b = W1[:, E:]
    _lib.checked().gdl_chan_weights_fwd(_p(pos), Cn, PD, HD, E, H1, _p(W0), _p(_f32vec(b0, HD, "weight_gen.0.bias")),
                                        _p(W2), _p(_f32vec(b2, E, "weight_gen.2.bias")), _p(w1b), W1.stride(0),
                                        _p(_f32vec(b1, H1, "channel_attention.0.bias")), _p(hid), _p(cw), _p(hb),
                                        _stream())
    return hid, cw, hb


def chan_weights_bwd(pos: Tensor, W2: Tensor, hid: Tensor, cw: Tensor, dcw: Tensor, dhb: Tensor):
    """-> (dW0 [HD,PD], db0, dW2 [E,HD], db2, dW1b [H1,PD], db1)"""
    _need_cuda(pos, dcw, dhb)
    Cn, PD = pos.shape
    HD, E, H1 = hid.shape[1], cw.shape[1], dhb.shape[1]
    _f32c(dcw, (Cn, E), "dcw"), _f32c(dhb, (Cn, H1), "dhb"), _f32c(W2, (E, HD), "weight_gen.2.weight")
    dev = pos.device
    outs = [torch.empty(sh, device=dev, dtype=torch.float32) for sh in ((HD, PD), (HD,), (E, HD), (E,), (H1, PD), (H1,))]
    _lib.checked().gdl_chan_weights_bwd(_p(pos), Cn, PD, HD, E, H1, _p(W2), _p(hid), _p(cw), _p(dcw), _p(dhb),
                                        *[_p(o) for o in outs], _stream())
    return tuple(outs)


def chan_pool(conv: Tensor, cw: Tensor, W1: Tensor, hb: Tensor, w2: Tensor, b2s: float):
    """conv [B, C, P, E] f32 -> (agg [B, P, E] f32, attn [B, P, C]) (mix_transformer.py:823-853)."""
    _need_cuda(conv, cw, W1, hb, w2)
    B, Cn, P, E = conv.shape
    H1 = hb.shape[1]
    _f32c(conv, (B, Cn, P, E), "conv"), _f32c(cw, (Cn, E), "cw"), _f32c(hb, (Cn, H1), "hb")
    if W1.dtype != torch.float32 or W1.shape[0] != H1 or W1.shape[1] < E or W1.stride(1) != 1:
        raise ValueError("chan_pool: W1 must be f32 [H1, >= E] with unit column stride")
    agg = torch.empty((B, P, E), device=conv.device, dtype=torch.float32)
    attn = torch.empty((B, P, Cn), device=conv.device, dtype=torch.float32)
    _lib.checked().gdl_chan_pool_fwd(_p(conv), B, Cn, P, E, H1, _p(cw), _p(W1), W1.stride(0), _p(hb),
                                     _p(_f32vec(w2, H1, "channel_attention.2.weight")), float(b2s), _p(agg), _p(attn),
                                     _stream())
    return agg, attn


def chan_pool_bwd(conv: Tensor, cw: Tensor, W1: Tensor, hb: Tensor, w2: Tensor, b2s: float, dagg: Tensor):
    """-> (dconv like conv, dW1a [H1,E], dhb [C,H1], dw2 [H1], dcw [C,E])"""
    _need_cuda(conv, dagg)
    B, Cn, P, E = conv.shape
    H1 = hb.shape[1]
    _f32c(dagg, (B, P, E), "dagg")
    lib = _lib.checked()
    nbytes = lib.gdl_chan_pool_workspace(B, Cn, P, E, H1)
    ws = torch.empty(max(nbytes, 4) // 4, device=conv.device, dtype=torch.float32)
    dconv = torch.empty_like(conv)
    grads = torch.empty(H1 * E + Cn * H1 + H1 + Cn * E, device=conv.device, dtype=torch.float32)
    lib.gdl_chan_pool_bwd(_p(conv), B, Cn, P, E, H1, _p(cw), _p(W1), W1.stride(0), _p(hb), _p(w2), float(b2s),
                          _p(dagg), _p(dconv), _p(grads), _p(ws), nbytes, _stream())
    o1, o2, o3 = H1 * E, H1 * E + Cn * H1, H1 * E + Cn * H1 + H1
    return dconv, grads[:o1].view(H1, E), grads[o1:o2].view(Cn, H1), grads[o2:o3], grads[o3:].view(Cn, E)


def col2im(cols: Tensor, B: int, Ho: int, Wo: int, R: int, S: int, Cc: int, stride: int, pad: int, H: int, W: int,
           out_dtype: torch.dtype) -> Tensor:
    """cols [B*Ho*Wo, R*S*C] -> dx NHWC [B,H,W,C] (data gradient of a strided conv)."""
    _need_cuda(cols)
    if not cols.is_contiguous() or cols.numel() != B * Ho * Wo * R * S * Cc:
        raise ValueError("col2im: contiguous [B*Ho*Wo, R*S*C] expected")
    dx = torch.empty((B, H, W, Cc), device=cols.device, dtype=out_dtype)
    _lib.checked().gdl_col2im(_p(cols), dt(cols), B, Ho, Wo, R, S, Cc, stride, pad, H, W, _p(dx), dt(dx),
                              dx.stride(0), dx.stride(1), dx.stride(2), _stream())
    return dx


def _bgemm(inp: Tensor, in_sW: int, in_sZ: tuple[int, int], w: Tensor, w_sN: int, w_sZ: tuple[int, int], out: Tensor,
           out_sW: int, out_sZ: tuple[int, int], M: int, K: int, N: int, nz: int, nz_inner: int, alpha: float) -> None:
    """out[z][m, n] = alpha * sum_k in[z][m, k] * w[z][n, k] over nz = (z0, z1) problems."""
    a = ConvArgs()
    a.inp, a.dtype = inp.data_ptr(), dt(inp)
    a.B, a.H, a.W, a.C = 1, 1, M, K
    a.in_sB, a.in_sH, a.in_sW = M * in_sW, M * in_sW, in_sW
    a.Ho, a.Wo, a.R, a.S, a.stride, a.pad = 1, M, 1, 1, 1, 0
    a.w, a.w_sN, a.N = w.data_ptr(), w_sN, N
    a.out, a.out_dtype = out.data_ptr(), dt(out)
    a.out_sB, a.out_sH, a.out_sW = M * out_sW, M * out_sW, out_sW
    a.alpha, a.act = alpha, ACT_NONE
    a.nz, a.nz_inner = nz, nz_inner
    a.in_sZ0, a.in_sZ1 = in_sZ
    a.w_sZ0, a.w_sZ1 = w_sZ
    a.out_sZ0, a.out_sZ1 = out_sZ
    batched_gemm_raw(a)


def _bwgrad(x: Tensor, x_sW: int, x_sZ: tuple[int, int], dy: Tensor, dy_sW: int, dy_sZ: tuple[int, int], dw: Tensor,
            P: int, Cc: int, N: int, nz: int, nz_inner: int) -> None:
    """dw[z][n, c] = sum_p dy[z][p, n] * x[z][p, c] (f32), dw dense [nz, N, C]."""
    a = WgradArgs()
    a.inp, a.dy, a.dtype = x.data_ptr(), dy.data_ptr(), dt(x)
    a.B, a.H, a.W, a.C = 1, 1, P, Cc
    a.in_sB, a.in_sH, a.in_sW = P * x_sW, P * x_sW, x_sW
    a.Ho, a.Wo, a.R, a.S, a.stride, a.pad, a.N = 1, P, 1, 1, 1, 0, N
    a.dy_sB, a.dy_sH, a.dy_sW = P * dy_sW, P * dy_sW, dy_sW
    a.dw, a.dw_sN, a.accumulate = dw.data_ptr(), Cc, 0
    a.nz, a.nz_inner = nz, nz_inner
    a.in_sZ0, a.in_sZ1 = x_sZ
    a.dy_sZ0, a.dy_sZ1 = dy_sZ
    a.dw_sZ0, a.dw_sZ1 = nz_inner * N * Cc, N * Cc
    lib = _lib.load()
    nbytes = lib.gdl_conv_wgrad_workspace(C.byref(a))      # nz * splits partials: batched problems are split too (up to 64 ways)
    ws = torch.empty(max(nbytes, 4) // 4, device=x.device, dtype=torch.float32)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    check(lib.gdl_conv_wgrad(C.byref(a), _stream()), "gdl_conv_wgrad(batched)")


def attention_bwd(q: Tensor, k: Tensor, v: Tensor, do: Tensor, num_heads: int, dq: Tensor, dk: Tensor,
                  dv: Tensor, o: Tensor | None = None, lse: Tensor | None = None) -> None:
    """Backward of softmax(q k^T / sqrt(hd)) v.  q/do/dq [B,Nq,D], k/v/dk/dv [B,Nkv,D]; all may be strided
    slices of packed qkv / kv tensors (unit channel stride); dq/dk/dv are written in place.

    With the forward's output ``o`` and ``lse`` (bf16, head_dim 64) the fused kernels run (nothing of size Nq x Nkv in
    HBM); otherwise -- the exact-f32 parity path and odd head dims -- the materialised path below.

    The probabilities are recomputed (the forward is the fused flash kernel and keeps none):
    S = scale q k^T -> P = softmax(S); dP = dO V^T; dS = P*(dP - rowsum(dP*P))*scale;
    dQ = dS K (batched GEMM against K^T); dK = dS^T Q, dV = P^T dO (batched weight-gradient kernels)."""
    B, Nq, Nkv, D, hd = _attn_check(q, k, v, num_heads)
    if o is not None and lse is not None and flash_ok(q, num_heads):
        attention_flash_bwd(q, k, v, o, do, lse, num_heads, dq, dk, dv)
        return
    cdt = q.dtype
    al = 4 if cdt == torch.float32 else 8
    if hd % al != 0:
        raise ValueError(f"attention_bwd: head_dim {hd} must be a multiple of {al} for {cdt}")
    for t, n in ((do, Nq), (dq, Nq), (dk, Nkv), (dv, Nkv)):
        if t.shape != (B, n, D) or t.dtype != cdt or t.stride(2) != 1:
            raise ValueError("attention_bwd: gradient tensor shape / dtype / stride mismatch")
    Hh = num_heads
    npad = (Nkv + 63) // 64 * 64
    lib = _lib.checked()
    nz = B * Hh
    sc_z = (Hh * Nq * npad, Nq * npad)
    scale = float(hd) ** -0.5
    P = torch.empty((B, Hh, Nq, npad), device=q.device, dtype=cdt)
    _bgemm(q, q.stride(1), (q.stride(0), hd), k, k.stride(1), (k.stride(0), hd), P, npad, sc_z, Nq, hd, Nkv, nz, Hh,
           scale)
    lib.gdl_softmax_rows(_p(P), _p(P), dt(P), nz * Nq, Nkv, npad, _stream())
    dS = torch.empty_like(P)
    _bgemm(do, do.stride(1), (do.stride(0), hd), v, v.stride(1), (v.stride(0), hd), dS, npad, sc_z, Nq, hd, Nkv, nz, Hh,
           1.0)
    lib.gdl_softmax_bwd_rows(_p(P), _p(dS), _p(dS), dt(P), nz * Nq, Nkv, npad, scale, _stream())
    kt = _v_transposed(k, Hh, hd, npad)                                    # K^T [B,H,hd,npad]
    _bgemm(dS, npad, sc_z, kt, npad, (Hh * hd * npad, hd * npad), dq, dq.stride(1), (dq.stride(0), hd), Nq, npad, hd,
           nz, Hh, 1.0)
    dkv32 = torch.empty((2, B, Hh, npad, hd), device=q.device, dtype=torch.float32)
    _bwgrad(q, q.stride(1), (q.stride(0), hd), dS, npad, sc_z, dkv32[0], Nq, hd, npad, nz, Hh)
    _bwgrad(do, do.stride(1), (do.stride(0), hd), P, npad, sc_z, dkv32[1], Nq, hd, npad, nz, Hh)
    for src, dst in ((dkv32[0], dk), (dkv32[1], dv)):
        # [B,H,n,hd] f32 -> [B,n,H*hd] slice in the compute dtype: a strided copy-cast (identity resample)
        bilinear(src.permute(0, 2, 1, 3)[:, :Nkv], (Nkv, Hh),
                 out=dst.as_strided((B, Nkv, Hh, hd), (dst.stride(0), dst.stride(1), hd, 1)))


# ------------------------------------------------------------------ ResNet / UNet++ pieces
def maxpool3x3s2(x: Tensor) -> Tensor:
    """F.max_pool2d(kernel 3, stride 2, padding 1) on NHWC."""
    _need_cuda(x)
    x4 = _nhwc4(x, "maxpool x")
    B, H, W, Cc = x4.shape
    out = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc), device=x.device, dtype=x.dtype)
    _lib.checked().gdl_maxpool3x3s2_fwd(_p(x4), dt(x4), B, H, W, Cc, x4.stride(0), x4.stride(1), x4.stride(2), _p(out),
                                        out.stride(0), out.stride(1), out.stride(2), _stream())
    return out


def maxpool3x3s2_bwd(x: Tensor, dout: Tensor) -> Tensor:
    x4, d4 = _nhwc4(x, "maxpool_bwd x"), _nhwc4(dout, "maxpool_bwd dout")
    B, H, W, Cc = x4.shape
    din = torch.empty((B, H, W, Cc), device=x.device, dtype=x.dtype)
    _lib.checked().gdl_maxpool3x3s2_bwd(_p(x4), _p(d4), _p(din), dt(x4), B, H, W, Cc, x4.stride(0), x4.stride(1),
                                        x4.stride(2), d4.stride(0), d4.stride(1), d4.stride(2), din.stride(0),
                                        din.stride(1), din.stride(2), _stream())
    return din


def maxpool2x2s2(x: Tensor) -> Tensor:
    """F.max_pool2d(kernel 2, stride 2) on NHWC (floor output size: an odd last row / column is dropped)."""
    _need_cuda(x)
    x4 = _nhwc4(x, "maxpool2x2 x")
    B, H, W, Cc = x4.shape
    if H < 2 or W < 2:
        raise ValueError(f"maxpool2x2s2: the map must be at least 2 x 2, got {H} x {W}")
    out = torch.empty((B, H // 2, W // 2, Cc), device=x.device, dtype=x.dtype)
    _lib.checked().gdl_maxpool2x2s2_fwd(_p(x4), dt(x4), B, H, W, Cc, x4.stride(0), x4.stride(1), x4.stride(2), _p(out),
                                        out.stride(0), out.stride(1), out.stride(2), _stream())
    return out


def maxpool2x2s2_bwd(x: Tensor, dout: Tensor) -> Tensor:
    """Gradient of maxpool2x2s2 wrt x: each window's gradient goes to its first maximum, everything else is zero."""
    _need_cuda(x, dout)
    x4, d4 = _nhwc4(x, "maxpool2x2_bwd x"), _nhwc4(dout, "maxpool2x2_bwd dout")
    B, H, W, Cc = x4.shape
    if tuple(d4.shape) != (B, H // 2, W // 2, Cc) or d4.dtype != x4.dtype:
        raise ValueError(f"maxpool2x2s2_bwd: dout {tuple(d4.shape)} {d4.dtype} does not match x {tuple(x4.shape)} {x4.dtype}")
    din = torch.empty((B, H, W, Cc), device=x.device, dtype=x.dtype)
    _lib.checked().gdl_maxpool2x2s2_bwd(_p(x4), _p(d4), _p(din), dt(x4), B, H, W, Cc, x4.stride(0), x4.stride(1),
                                        x4.stride(2), d4.stride(0), d4.stride(1), d4.stride(2), din.stride(0),
                                        din.stride(1), din.stride(2), _stream())
    return din


def nearest2x(x: Tensor, out: Tensor | None = None) -> Tensor:
    """F.interpolate(scale_factor=2, mode='nearest') on NHWC; ``out`` may be a channel slice of a concat buffer."""
    _need_cuda(x)
    x4 = _nhwc4(x, "nearest2x x")
    B, H, W, Cc = x4.shape
    if out is None:
        out = torch.empty((B, 2 * H, 2 * W, Cc), device=x.device, dtype=x.dtype)
    o4 = _nhwc4(out, "nearest2x out")
    if tuple(o4.shape) != (B, 2 * H, 2 * W, Cc) or o4.dtype != x4.dtype:
        raise ValueError("nearest2x: out shape / dtype mismatch")
    _lib.checked().gdl_nearest2x_fwd(_p(x4), dt(x4), B, H, W, Cc, x4.stride(0), x4.stride(1), x4.stride(2), _p(o4),
                                     o4.stride(0), o4.stride(1), o4.stride(2), _stream())
    return out


def nearest2x_bwd(dout: Tensor) -> Tensor:
    d4 = _nhwc4(dout, "nearest2x_bwd dout")
    B, H2, W2, Cc = d4.shape
    din = torch.empty((B, H2 // 2, W2 // 2, Cc), device=dout.device, dtype=dout.dtype)
    _lib.checked().gdl_nearest2x_bwd(_p(d4), dt(d4), B, H2 // 2, W2 // 2, Cc, d4.stride(0), d4.stride(1), d4.stride(2),
                                     _p(din), din.stride(0), din.stride(1), din.stride(2), _stream())
    return din


def add_relu(a: Tensor, b: Tensor) -> Tensor:
    if a.shape != b.shape or a.dtype != b.dtype or not a.is_contiguous() or not b.is_contiguous():
        raise ValueError("add_relu: two contiguous tensors of one shape / dtype expected")
    out = torch.empty_like(a)
    _lib.checked().gdl_add_relu(_p(a), _p(b), _p(out), dt(a), a.numel(), _stream())
    return out


def pad_channels(x: Tensor, cpad: int, out_dtype: torch.dtype) -> Tensor:
    """Dense [..., C] -> [..., cpad] in out_dtype with zero-filled extra channels."""
    _need_cuda(x)
    if not x.is_contiguous():
        raise ValueError("pad_channels: contiguous input expected")
    Cc = x.shape[-1]
    out = torch.empty((*x.shape[:-1], cpad), device=x.device, dtype=out_dtype)
    _lib.checked().gdl_pad_channels(_p(x), dt(x), x.numel() // Cc, Cc, _p(out), dt(out), cpad, _stream())
    return out


def relu_bwd(y: Tensor, dy: Tensor) -> Tensor:
    if y.shape != dy.shape or y.dtype != dy.dtype or not y.is_contiguous() or not dy.is_contiguous():
        raise ValueError("relu_bwd: two contiguous tensors of one shape / dtype expected")
    dx = torch.empty_like(y)
    _lib.checked().gdl_relu_bwd(_p(y), _p(dy), _p(dx), dt(y), y.numel(), _stream())
    return dx


# ------------------------------------------------------------------ DOFA patch embed helpers
def patchify(img: Tensor, P: int, pad: int, gh: int, gw: int, kpad: int,
             out_dtype: torch.dtype, stride: int | None = None) -> Tensor:
    _need_cuda(img)
    if img.dtype != torch.float32 or not img.is_contiguous():
        raise ValueError("patchify: image must be contiguous f32 NCHW")
    B, Cc, H, W = img.shape
    cols = torch.empty((B * gh * gw, kpad), device=img.device, dtype=out_dtype)
    _lib.checked().gdl_patchify(_p(img), B, Cc, H, W, P, P if stride is None else stride, pad, gh, gw,
                                _p(cols), dt(cols), kpad, _stream())
    return cols


def dofa_pack_kernel(g: Tensor, Cc: int, PP: int, D: int, scaler: float, kpad: int,
                     out_dtype: torch.dtype) -> Tensor:
    if g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != Cc * PP * D:
        raise ValueError("dofa_pack_kernel: g must be contiguous f32 [C, P*P*D]")
    out = torch.empty((D, kpad), device=g.device, dtype=out_dtype)
    _lib.checked().gdl_dofa_pack_kernel(_p(g), Cc, PP, D, scaler, _p(out), dt(out), kpad,
                                        _stream())
    return out


_OMEGA: dict = {}


def dofa_unpack_grad(dw: Tensor, Cc: int, PP: int, D: int, scaler: float) -> Tensor:
    """f32 [D, Kpad] gradient of the packed patch-embed weight -> [C, PP*D] gradient of the generated kernel."""
    if dw.dtype != torch.float32 or not dw.is_contiguous() or dw.shape[0] != D:
        raise ValueError("dofa_unpack_grad: contiguous f32 [D, Kpad] expected")
    dg = torch.empty((Cc, PP * D), device=dw.device, dtype=torch.float32)
    _lib.checked().gdl_dofa_unpack_grad(_p(dw), Cc, PP, D, scaler, dw.shape[1], _p(dg), _stream())
    return dg


def sincos_embed(pos: Tensor, D: int) -> Tensor:
    """position_embedding(D, pos) (dofa_v2.py:9-35); the frequency table is a host constant."""
    _need_cuda(pos)
    pos = pos.reshape(-1).contiguous().float()
    key = (D, pos.device)
    if key not in _OMEGA:
        omega = torch.arange(D // 2, dtype=torch.float32)
        omega /= D / 2.0
        _OMEGA[key] = (1.0 / 10000**omega).to(pos.device)
    out = torch.empty((pos.numel(), D), device=pos.device, dtype=torch.float32)
    _lib.checked().gdl_sincos_embed(_p(pos), _p(_OMEGA[key]), pos.numel(), D, _p(out), _stream())
    return out


def bn_fold(gamma: Tensor, beta: Tensor, mean: Tensor, var: Tensor, eps: float):
    Cc = gamma.numel()
    scale = torch.empty(Cc, device=gamma.device, dtype=torch.float32)
    shift = torch.empty_like(scale)
    _lib.checked().gdl_bn_fold(_p(gamma), _p(beta), _p(mean), _p(var), eps, Cc, _p(scale),
                               _p(shift), _stream())
    return scale, shift


def pack_dgrad(w: Tensor, N: int, T: int, Cc: int, out_dtype: torch.dtype) -> Tensor:
    """[N, T*C] forward weights -> [C, T*N] flipped/transposed weights for the data gradient."""
    if not w.is_contiguous() or w.numel() != N * T * Cc:
        raise ValueError("pack_dgrad: contiguous [N, T*C] weights expected")
    out = torch.empty((Cc, T * N), device=w.device, dtype=out_dtype)
    _lib.checked().gdl_pack_dgrad(_p(w), dt(w), N, T, Cc, _p(out), dt(out), _stream())
    return out


# ------------------------------------------------------------------ elementwise
def cast(x: Tensor, dtype: torch.dtype, out: Tensor | None = None) -> Tensor:
    _need_cuda(x)
    if not x.is_contiguous():
        raise ValueError("cast: contiguous input required")
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=dtype)
    _lib.checked().gdl_cast(_p(x), dt(x), _p(out), dt(out), x.numel(), _stream())
    return out


def scale_f32(x: Tensor, s: float) -> Tensor:
    out = torch.empty_like(x)
    _lib.checked().gdl_scale_f32(_p(x), _p(out), x.numel(), s, _stream())
    return out


def add_rows(a: Tensor, b: Tensor | None, out: Tensor, rows: int) -> Tensor:
    """out[r,:] = a[r % a_rows,:] + (b[r % b_rows,:] if b is given); 2-D f32 tensors."""
    D = a.shape[-1]
    _lib.checked().gdl_add_rows(_p(a), a.shape[0], a.stride(0), _p(b),
                                0 if b is None else b.shape[0], 0 if b is None else b.stride(0),
                                _p(out), out.stride(0), rows, D, _stream())
    return out


def normalize_u8(u8: Tensor, mean: Tensor, std: Tensor) -> Tensor:
    """uint8 NCHW -> (x/255 - mean[c]) / std[c] f32 (utils/tensors.py:10-35)."""
    _need_cuda(u8)
    if u8.dtype != torch.uint8 or not u8.is_contiguous():
        raise ValueError("normalize_u8: contiguous uint8 NCHW expected")
    B, Cc, H, W = u8.shape
    out = torch.empty((B, Cc, H, W), device=u8.device, dtype=torch.float32)
    _lib.checked().gdl_normalize_u8(_p(u8), _p(out), B, Cc, H * W, _p(_f32vec(mean, Cc, "mean")),
                                    _p(_f32vec(std, Cc, "std")), _stream())
    return out


_RAW_KIND = {torch.uint8: 0, torch.uint16: 1, torch.int16: 2, torch.float32: 3}


def normalize_raw(raw: Tensor, mean: Tensor, std: Tensor) -> Tensor:
    """Raw NCHW samples (uint8 / uint16 / int16 / f32) -> (float(x)/255 - mean[c]) / std[c] f32
    (datasets/wds_dataset.py:230-236 + utils/tensors.py:10-35)."""
    _need_cuda(raw)
    if raw.dtype not in _RAW_KIND or not raw.is_contiguous() or raw.dim() != 4:
        raise ValueError(f"normalize_raw: contiguous NCHW uint8/uint16/int16/float32 expected, got {raw.dtype}")
    B, Cc, H, W = raw.shape
    out = torch.empty((B, Cc, H, W), device=raw.device, dtype=torch.float32)
    _lib.checked().gdl_normalize_raw(_p(raw), _RAW_KIND[raw.dtype], _p(out), B, Cc, H * W,
                                     _p(_f32vec(mean, Cc, "mean")), _p(_f32vec(std, Cc, "std")), _stream())
    return out


def normalize_range(raw: Tensor, mean: Tensor, std: Tensor, image_min: int = 0, image_max: int = 255, norm_min: float = 0.0,
                    norm_max: float = 1.0) -> Tensor:
    """Raw NCHW samples (uint8 / uint16 / int16 / f32) -> ((norm_max - norm_min) * (float(x) - image_min) / (image_max - image_min)
    + norm_min - mean[c]) / std[c] f32: ``normalization`` with the caller's sensor range, then ``standardization``
    (utils/tensors.py:10-35), every step in f32 in the reference's order."""
    if raw.dtype not in _RAW_KIND or not raw.is_contiguous() or raw.dim() != 4:
        raise ValueError(f"normalize_range: contiguous NCHW uint8/uint16/int16/float32 expected, got {raw.dtype}")
    if int(image_max) == int(image_min):
        raise ValueError(f"normalize_range: image_max == image_min ({int(image_min)}): the range is empty")
    _need_cuda(raw)
    B, Cc, H, W = raw.shape
    out = torch.empty((B, Cc, H, W), device=raw.device, dtype=torch.float32)
    _lib.checked().gdl_normalize_range(_p(raw), _RAW_KIND[raw.dtype], _p(out), B, Cc, H * W, int(image_min), int(image_max),
                                       float(norm_min), float(norm_max), _p(_f32vec(mean, Cc, "mean")),
                                       _p(_f32vec(std, Cc, "std")), _stream())
    return out


def augment(img: Tensor, mask: Tensor | None, params: Tensor, mean: Tensor | None = None,
            std: Tensor | None = None) -> tuple[Tensor, Tensor | None]:
    """Per-sample flip / rot90 / resized-crop of an NCHW tile (+ its int64 mask), optionally fused with the
    /255 + standardise of a raw tile.  ``params``: f32 [B, 8] = {kind, k, y0, x0, h, w, -, -} on the device."""
    _need_cuda(img, params)
    if img.dtype not in _RAW_KIND or not img.is_contiguous() or img.dim() != 4:
        raise ValueError("augment: contiguous NCHW uint8/uint16/int16/float32 tile expected")
    B, Cc, H, W = img.shape
    if params.shape != (B, 8) or params.dtype != torch.float32 or not params.is_contiguous():
        raise ValueError("augment: params must be a contiguous f32 [B, 8] tensor")
    out = torch.empty((B, Cc, H, W), device=img.device, dtype=torch.float32)
    m2 = om = None
    if mask is not None:
        if mask.dtype != torch.int64 or mask.numel() != B * H * W:
            raise ValueError("augment: int64 mask of B*H*W elements expected")
        m2 = mask.contiguous()
        om = torch.empty_like(m2)
    _lib.checked().gdl_augment(_p(img), _RAW_KIND[img.dtype], _p(out), _p(m2), _p(om), B, Cc, H, W,
                               _p(None if mean is None else _f32vec(mean, Cc, "mean")),
                               _p(None if std is None else _f32vec(std, Cc, "std")), _p(params), _stream())
    return out, om


def scale_outer(x: Tensor, s: Tensor) -> Tensor:
    """x[o, ...] *= s[o] in place."""
    if not x.is_contiguous():
        raise ValueError("scale_outer: contiguous tensor required")
    outer = x.shape[0]
    _lib.checked().gdl_scale_outer(_p(x), dt(x), _p(_f32vec(s, outer, "s")), outer,
                                   x.numel() // outer, _stream())
    return x


# ------------------------------------------------------------------ classifier tail
def head_1x1(feat: Tensor, w: Tensor, bias: Tensor | None, chan_scale: Tensor | None = None) -> Tensor:
    """NHWC features -> f32 NHWC logits [B,H,W,K] (K <= 16)."""
    f4 = _nhwc4(feat, "head feat")
    B, H, W, Cc = f4.shape
    P, _, sP = _pix(f4, "head feat")
    K = w.shape[0]
    w2 = w.reshape(K, Cc)
    if w2.dtype != torch.float32 or not w2.is_contiguous():
        raise ValueError("head_1x1: weight must be contiguous f32 [K, C]")
    out = torch.empty((B, H, W, K), device=feat.device, dtype=torch.float32)
    _lib.checked().gdl_head_1x1(_p(f4), dt(f4), P, Cc, sP, _p(w2), _p(bias), _p(chan_scale),
                                H * W, _p(out), K, _stream())
    return out


def head_1x1_bwd(feat: Tensor, dlog: Tensor, w: Tensor, chan_scale: Tensor | None,
                 need_dfeat: bool = True):
    f4 = _nhwc4(feat, "head feat")
    B, H, W, Cc = f4.shape
    P, _, sP = _pix(f4, "head feat")
    K = w.shape[0]
    w2 = w.reshape(K, Cc)
    dfeat = torch.empty((B, H, W, Cc), device=feat.device, dtype=feat.dtype) if need_dfeat else None
    dw = torch.empty((K, Cc), device=feat.device, dtype=torch.float32)
    db = torch.empty(K, device=feat.device, dtype=torch.float32)
    lib = _lib.checked()
    nbytes = lib.gdl_head_1x1_bwd_workspace(P, Cc, K)
    ws = torch.empty(nbytes // 4, device=feat.device, dtype=torch.float32)
    lib.gdl_head_1x1_bwd(_p(f4), dt(f4), _p(dlog), P, Cc, sP, _p(w2), _p(chan_scale), H * W,
                         _p(dfeat), Cc, _p(dw), _p(db), K, _p(ws), nbytes, _stream())
    return dfeat, dw, db


def _head_bn_args(x: Tensor, w: Tensor, who: str):
    x4 = _nhwc4(x, who)
    B, H, W, Cc = x4.shape
    if x4.dtype != torch.bfloat16 or not x4.is_contiguous():
        raise ValueError(f"{who}: dense bf16 NHWC map expected")
    K = w.shape[0]
    w2 = w.reshape(K, Cc)
    if w2.dtype != torch.float32 or not w2.is_contiguous():
        raise ValueError(f"{who}: weight must be contiguous f32 [K, C]")
    return x4, B * H * W, Cc, K, w2


def head_1x1_bn(x: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, beta: Tensor, eps: float, relu: bool, w: Tensor,
                bias: Tensor | None) -> Tensor:
    """head_1x1(bn_apply(x, ...), w, bias) without the normalised map: f32 NHWC logits [B,H,W,K] from the pre-BatchNorm bf16 map
    ``x`` (C == 256), bit-identical to the two separate ops."""
    _need_cuda(x, w)
    x4, P, Cc, K, w2 = _head_bn_args(x, w, "head_1x1_bn x")
    out = torch.empty((*x4.shape[:3], K), device=x.device, dtype=torch.float32)
    _lib.checked().gdl_head_1x1_bn(_p(x4), dt(x4), P, Cc, _p(_f32vec(mean, Cc, "mean")), _p(_f32vec(var, Cc, "var")),
                                   _p(_f32vec(gamma, Cc, "gamma")), _p(_f32vec(beta, Cc, "beta")), eps, int(relu), _p(w2),
                                   _p(bias), _p(out), K, _stream())
    return out


def bn_head_bwd_reduce(x: Tensor, dlog: Tensor, w: Tensor, mean, var, gamma, beta, eps, relu):
    """(dgamma, dbeta, dw [K, C], db [K]) of head_1x1(relu?(bn(x))) from the head's logit gradient ``dlog`` [B,H,W,K] f32: the sums
    of bn_bwd_reduce and the parameter gradients of head_1x1_bwd in one read of ``x``."""
    _need_cuda(x, dlog, w)
    x4, P, Cc, K, w2 = _head_bn_args(x, w, "bn_head_bwd x")
    if dlog.dtype != torch.float32 or not dlog.is_contiguous() or dlog.numel() != P * K:
        raise ValueError("bn_head_bwd: dlog must be contiguous f32 [B, H, W, K]")
    dgamma = torch.empty(Cc, device=x.device, dtype=torch.float32)
    dbeta = torch.empty_like(dgamma)
    dw = torch.empty((K, Cc), device=x.device, dtype=torch.float32)
    db = torch.empty(K, device=x.device, dtype=torch.float32)
    lib = _lib.checked()
    nbytes = lib.gdl_bn_head_bwd_workspace(P, Cc, K)
    ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32)
    lib.gdl_bn_head_bwd_reduce(_p(x4), dt(x4), _p(dlog), P, Cc, K, _p(w2), _p(_f32vec(mean, Cc, "mean")), _p(_f32vec(var, Cc, "var")),
                               _p(_f32vec(gamma, Cc, "gamma")), _p(_f32vec(beta, Cc, "beta")), eps,
                               int(relu), _p(dgamma), _p(dbeta), _p(dw), _p(db), _p(ws), nbytes, _stream())
    return dgamma, dbeta, dw, db


def bn_head_bwd_dx(x: Tensor, dlog: Tensor, w: Tensor, mean, var, gamma, beta, eps, relu, dgamma_sum, dbeta_sum, p_total,
                   out: Tensor | None = None) -> Tensor:
    """bn_bwd_dx with the gradient of the normalised map re-formed from the head's logit gradient; ``out`` may be ``x``."""
    _need_cuda(x, dlog, w)
    x4, P, Cc, K, w2 = _head_bn_args(x, w, "bn_head_bwd x")
    if dlog.dtype != torch.float32 or not dlog.is_contiguous() or dlog.numel() != P * K:
        raise ValueError("bn_head_bwd: dlog must be contiguous f32 [B, H, W, K]")
    dx = out if out is not None else torch.empty(x.shape, device=x.device, dtype=x.dtype)
    if dx.dtype != x.dtype or dx.shape != x.shape or not dx.is_contiguous():
        raise ValueError("bn_head_bwd_dx: out must be a dense map of x's shape and dtype")
    _lib.checked().gdl_bn_head_bwd_dx(_p(x4), dt(x4), _p(dlog), _p(dx), P, Cc, K, _p(w2), _p(_f32vec(mean, Cc, "mean")),
                                      _p(_f32vec(var, Cc, "var")), _p(_f32vec(gamma, Cc, "gamma")), _p(_f32vec(beta, Cc, "beta")),
                                      eps, int(relu), _p(_f32vec(dgamma_sum, Cc, "dgamma_sum")), _p(_f32vec(dbeta_sum, Cc, "dbeta_sum")),
                                      p_total, _stream())
    return dx


def upsample_logits(x: Tensor, size: tuple[int, int]) -> Tensor:
    """f32 NHWC [B,Hi,Wi,K] -> NCHW f32 [B,K,Ho,Wo] (bilinear, align_corners=False)."""
    B, Hi, Wi, K = x.shape
    out = torch.empty((B, K, size[0], size[1]), device=x.device, dtype=torch.float32)
    _lib.checked().gdl_upsample_logits(_p(x), B, Hi, Wi, K, _p(out), size[0], size[1], _stream())
    return out


def upsample_logits_bwd(dout: Tensor, in_size: tuple[int, int]) -> Tensor:
    if dout.dtype != torch.float32 or not dout.is_contiguous():
        raise ValueError("upsample_logits_bwd: contiguous f32 NCHW grad expected")
    B, K, Ho, Wo = dout.shape
    din = torch.empty((B, in_size[0], in_size[1], K), device=dout.device, dtype=torch.float32)
    lib = _lib.checked()
    nbytes = lib.gdl_upsample_logits_bwd_workspace(B, K, in_size[0], Wo)
    ws = torch.empty(nbytes // 4, device=dout.device, dtype=torch.float32)
    lib.gdl_upsample_logits_bwd(_p(dout), B, Ho, Wo, K, _p(din), in_size[0], in_size[1], _p(ws),
                                nbytes, _stream())
    return din


def softmax_argmax(logits: Tensor) -> Tensor:
    """softmax(dim=1).argmax(dim=1) on NCHW f32 logits -> int64 [B,H,W]."""
    _need_cuda(logits)
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("softmax_argmax: contiguous f32 NCHW logits expected")
    B, K, H, W = logits.shape
    mask = torch.empty((B, H, W), device=logits.device, dtype=torch.int64)
    _lib.checked().gdl_softmax_argmax(_p(logits), B, K, H * W, _p(mask), _stream())
    return mask


def upsample_argmax(low: Tensor, size: tuple[int, int]) -> Tensor:
    """softmax(dim=1).argmax(dim=1) of bilinear(low -> size) for the head's NHWC f32 map [B, h, w, K] -> int64 [B, H, W], without the
    resized logits (gdl_upsample_argmax; the same mask as upsample_logits + softmax_argmax)."""
    _need_cuda(low)
    if low.dtype != torch.float32 or not low.is_contiguous() or low.dim() != 4 or not 2 <= low.shape[3] <= 16:
        raise ValueError("upsample_argmax: contiguous f32 NHWC logits [B, h, w, K] with 2..16 classes expected")
    B, Hi, Wi, K = low.shape
    mask = torch.empty((B, int(size[0]), int(size[1])), device=low.device, dtype=torch.int64)
    _lib.checked().gdl_upsample_argmax(_p(low), B, Hi, Wi, K, _p(mask), int(size[0]), int(size[1]), _stream())
    return mask


def sigmoid_threshold(logits: Tensor, threshold: float = 0.5) -> Tensor:
    """``(logits.sigmoid() > threshold).long()`` (segmentation_dofa.py:279) in one pass: f32 logits [B, 1, H, W] -> int64 [B, H, W];
    any other shape keeps its shape.  The comparison is made on the f32 sigmoid, as the reference makes it."""
    _need_cuda(logits)
    if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.numel() == 0:
        raise ValueError("sigmoid_threshold: contiguous f32 logits expected")
    shape = (logits.shape[0], *logits.shape[2:]) if logits.dim() == 4 and logits.shape[1] == 1 else tuple(logits.shape)
    mask = torch.empty(shape, device=logits.device, dtype=torch.int64)
    _lib.checked().gdl_sigmoid_threshold(_p(logits), logits.numel(), float(threshold), _p(mask), _stream())
    return mask


def _binary_lowres_check(who: str, low: Tensor, size: tuple[int, int], target: Tensor | None = None) -> tuple:
    """The shapes the one-class low-resolution entry points take, checked before anything touches the device: (B, Hi, Wi, Ho, Wo)."""
    if low.dim() != 4 or low.shape[3] != 1:
        raise ValueError(f"{who}: one-class NHWC low-resolution logits [B, h, w, 1] expected, got {tuple(low.shape)}")
    B, Hi, Wi, _ = low.shape
    Ho, Wo = int(size[0]), int(size[1])
    if B < 1 or Hi < 1 or Wi < 1 or Ho < Hi or Wo < Wi:
        raise ValueError(f"{who}: an upsample is expected, got {Hi} x {Wi} -> {Ho} x {Wo}")
    if -(-Ho // Hi) > 64 or -(-Wo // Wi) > 64:
        raise ValueError(f"{who}: upsampling factors above 64 are not supported, got {Hi} x {Wi} -> {Ho} x {Wo}")
    _need_cuda(low, target)
    if low.dtype != torch.float32 or not low.is_contiguous():
        raise ValueError(f"{who}: contiguous f32 low-resolution logits expected")
    if target is not None and (target.dtype != torch.int64 or not target.is_contiguous() or tuple(target.shape) != (B, Ho, Wo)):
        raise ValueError(f"{who}: contiguous int64 target {[B, Ho, Wo]} expected, got {tuple(target.shape)}")
    return B, Hi, Wi, Ho, Wo


# Largest upsampling factor (per direction) at which the one-class low-resolution loss kernels were measured faster than materialising
# the [B, 1, H, W] logits (tools/bench_binary_lowres.py -> profiles/bench_binary_lowres.txt: 0.90 x at factor 4, 0.95 x at 8, 1.06-1.10 x at 16, 1.10-1.17 x at 32;
# one shape only, batch 64 to 512^2, applied to every batch and output size): with
# one class the resized tensor is small, and at large factors a tile's transposed resize has few low-resolution logits to spread
# over its threads.
BINARY_LOWRES_MAX_FACTOR = 8


def binary_lowres_pays(low: Tensor, size: tuple[int, int]) -> bool:
    """Shapes for which a binary loss reads the one-class head's map [B, h, w, 1] instead of the resized logits: those the
    kernels take (dice_lowres_ok) with factors up to BINARY_LOWRES_MAX_FACTOR; beyond it the materialised path is the faster one."""
    if low.dim() != 4 or low.shape[3] != 1 or not dice_lowres_ok(low, size):
        return False
    return -(-size[0] // low.shape[1]) <= BINARY_LOWRES_MAX_FACTOR and -(-size[1] // low.shape[2]) <= BINARY_LOWRES_MAX_FACTOR


def upsample_threshold(low: Tensor, size: tuple[int, int], threshold: float = 0.5) -> Tensor:
    """``(bilinear(low -> size).sigmoid() > threshold).long()`` for the one-class head's NHWC f32 map [B, h, w, 1] -> int64
    [B, H, W], without the resized logits (gdl_upsample_threshold; the same mask as upsample_logits + sigmoid_threshold)."""
    B, Hi, Wi, Ho, Wo = _binary_lowres_check("upsample_threshold", low, size)
    mask = torch.empty((B, Ho, Wo), device=low.device, dtype=torch.int64)
    _lib.checked().gdl_upsample_threshold(_p(low), B, Hi, Wi, _p(mask), Ho, Wo, float(threshold), _stream())
    return mask


def class_probs(logits: Tensor) -> Tensor:
    """NCHW f32 logits -> softmax(dim=1) (or sigmoid for one class) probabilities."""
    _need_cuda(logits)
    if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() != 4:
        raise ValueError("class_probs: contiguous f32 NCHW logits expected")
    B, K, H, W = logits.shape
    out = torch.empty_like(logits)
    _lib.checked().gdl_class_probs(_p(logits), B, K, H * W, _p(out), _stream())
    return out


def upsample_probs(low: Tensor, size: tuple[int, int]) -> Tensor:
    """softmax(dim=1) (2..16 classes) or sigmoid (one class) of bilinear(low -> size) for a head's NHWC f32 map [B, h, w, K] -> f32
    [B, K, H, W], without the resized logits (gdl_upsample_probs; the probabilities of upsample_logits + class_probs)."""
    _need_cuda(low)
    if low.dtype != torch.float32 or not low.is_contiguous() or low.dim() != 4 or not 1 <= low.shape[3] <= 16:
        raise ValueError("upsample_probs: contiguous f32 NHWC logits [B, h, w, K] with 1..16 classes expected")
    B, Hi, Wi, K = low.shape
    Ho, Wo = int(size[0]), int(size[1])
    if min(B, Hi, Wi, Ho, Wo) < 1:
        raise ValueError(f"upsample_probs: bad sizes {tuple(low.shape)} -> {Ho} x {Wo}")
    out = torch.empty((B, K, Ho, Wo), device=low.device, dtype=torch.float32)
    _lib.checked().gdl_upsample_probs(_p(low), B, Hi, Wi, K, _p(out), Ho, Wo, _stream())
    return out


# ------------------------------------------------------------------ whole-scene inference (include/gdlhip_scene.h)
_RAW_LIMITS = {torch.uint8: (0, 255), torch.uint16: (0, 65535), torch.int16: (-32768, 32767)}


def _scene_origins(op: str, origins: Tensor) -> int:
    if origins.dtype != torch.int32 or origins.dim() != 2 or origins.shape[1] != 2 or origins.shape[0] < 1 or not origins.is_contiguous():
        raise ValueError(f"{op}: origins must be a contiguous int32 [B, 2] tensor of (y0, x0), got {origins.dtype} {tuple(origins.shape)}")
    return int(origins.shape[0])


def _scene_cut_check(op: str, raster: Tensor, origins: Tensor, xforms: Tensor | None, tile: tuple[int, int], mean: Tensor, std: Tensor,
                     image_min: int, image_max: int, fill: int, check_codes: bool = True) -> tuple[int, int, int]:
    """The argument checks of the three cuts, in one order; (B, th, tw)."""
    if raster.dtype not in _RAW_KIND or not raster.is_contiguous() or raster.dim() != 3:
        raise ValueError(f"{op}: contiguous [C, H, W] uint8/uint16/int16/float32 raster expected, got {raster.dtype} {tuple(raster.shape)}")
    if int(image_max) == int(image_min):
        raise ValueError(f"{op}: image_max == image_min ({int(image_min)}): the range is empty")
    _need_cuda(raster, origins, mean, std)
    B = _scene_origins(op, origins)
    th, tw = int(tile[0]), int(tile[1])
    if th < 1 or tw < 1:
        raise ValueError(f"{op}: bad tile {th} x {tw}")
    if xforms is not None:
        _scene_xforms(op, xforms, B, (th, tw), check_codes)
    lo, hi = _RAW_LIMITS.get(raster.dtype, (-2 ** 31, 2 ** 31 - 1))
    if not lo <= int(fill) <= hi:
        raise ValueError(f"{op}: fill {fill} is not a value of {raster.dtype}")
    return B, th, tw


def scene_cut(raster: Tensor, origins: Tensor, tile: tuple[int, int], mean: Tensor, std: Tensor, image_min: int = 0,
              image_max: int = 255, norm_min: float = 0.0, norm_max: float = 1.0, fill: int = 0) -> Tensor:
    """Normalised NCHW f32 tiles [B, C, th, tw] cut out of a raw raster [C, H, W] (uint8 / uint16 / int16 / f32) at the origins
    int32 [B, 2] = (y0, x0), which may be negative or reach past the raster: a position outside it takes the raw value ``fill``.
    The values are those of ``normalize_range`` on the sliced (and padded) tile, bit for bit (gdl_scene_cut)."""
    B, th, tw = _scene_cut_check("scene_cut", raster, origins, None, tile, mean, std, image_min, image_max, fill)
    Cc, H, W = raster.shape
    out = torch.empty((B, Cc, th, tw), device=raster.device, dtype=torch.float32)
    _lib.checked().gdl_scene_cut(_p(raster), _RAW_KIND[raster.dtype], Cc, H, W, _p(origins), B, th, tw, int(fill), _p(out),
                                 int(image_min), int(image_max), float(norm_min), float(norm_max), _p(_f32vec(mean, Cc, "mean")),
                                 _p(_f32vec(std, Cc, "std")), _stream())
    return out


def _scene_blend_check(op: str, src: Tensor, K: int, tile: tuple[int, int], origins: Tensor, wy: Tensor, wx: Tensor, canvas: Tensor,
                       box: tuple[int, int, int, int] | None) -> tuple[int, int, int, int, int, int]:
    _need_cuda(src, origins, wy, wx, canvas)
    if not 1 <= K <= 16:
        raise ValueError(f"{op}: 1..16 classes, got {K}")
    if _scene_origins(op, origins) != src.shape[0]:
        raise ValueError(f"{op}: {origins.shape[0]} origins for {src.shape[0]} tiles")
    th, tw = tile
    _f32vec(wy, th, f"{op}: the row window wy")
    _f32vec(wx, tw, f"{op}: the column window wx")
    if canvas.dtype != torch.float32 or canvas.dim() != 3 or canvas.shape[0] != K + 1 or not canvas.is_contiguous():
        raise ValueError(f"{op}: canvas must be a contiguous f32 [K+1, H, W] = [{K + 1}, H, W] tensor, got {canvas.dtype} {tuple(canvas.shape)}")
    H, W = int(canvas.shape[1]), int(canvas.shape[2])
    y0, y1, x0, x1 = (0, H, 0, W) if box is None else (int(v) for v in box)
    return H, W, y0, y1, x0, x1


def scene_blend(probs: Tensor, origins: Tensor, wy: Tensor, wx: Tensor, canvas: Tensor,
                box: tuple[int, int, int, int] | None = None) -> Tensor:
    """Adds the window-weighted probabilities [B, K, th, tw] f32 of the tiles at ``origins`` into ``canvas`` [K+1, H, W] f32 in
    place (plane K: the weights), over the canvas pixels of ``box`` = (y0, y1, x0, x1), the batch's bounding box (default: the
    whole canvas).  A gather in ascending tile order without atomics: the result does not depend on the batching (gdl_scene_blend)."""
    if probs.dtype != torch.float32 or probs.dim() != 4 or not probs.is_contiguous():
        raise ValueError("scene_blend: contiguous f32 probabilities [B, K, th, tw] expected")
    B, K, th, tw = probs.shape
    H, W, y0, y1, x0, x1 = _scene_blend_check("scene_blend", probs, K, (th, tw), origins, wy, wx, canvas, box)
    _lib.checked().gdl_scene_blend(_p(probs), B, K, th, tw, _p(origins), _p(wy), _p(wx), _p(canvas), H, W, y0, y1, x0, x1, _stream())
    return canvas


def scene_blend_lowres(low: Tensor, size: tuple[int, int], origins: Tensor, wy: Tensor, wx: Tensor, canvas: Tensor,
                       box: tuple[int, int, int, int] | None = None) -> Tensor:
    """``scene_blend`` of ``upsample_probs(low, size)`` without those probabilities: each tile pixel's softmax (2..16 classes) or
    sigmoid (one class) is evaluated from the head's NHWC f32 map [B, h, w, K] where it is added (gdl_scene_blend_lowres)."""
    if low.dtype != torch.float32 or low.dim() != 4 or not low.is_contiguous():
        raise ValueError("scene_blend_lowres: contiguous f32 NHWC logits [B, h, w, K] expected")
    B, hi, wi, K = low.shape
    th, tw = int(size[0]), int(size[1])
    if min(hi, wi, th, tw) < 1:
        raise ValueError(f"scene_blend_lowres: bad sizes {tuple(low.shape)} -> {th} x {tw}")
    H, W, y0, y1, x0, x1 = _scene_blend_check("scene_blend_lowres", low, K, (th, tw), origins, wy, wx, canvas, box)
    _lib.checked().gdl_scene_blend_lowres(_p(low), B, hi, wi, K, th, tw, _p(origins), _p(wy), _p(wx), _p(canvas), H, W, y0, y1, x0, x1,
                                          _stream())
    return canvas


# test-time augmentation (include/gdlhip_scene_tta.h): the cut and the two blends with a transform code per tile
def _scene_xforms(op: str, xforms: Tensor, B: int, tile: tuple[int, int], check_codes: bool) -> None:
    """``xforms``: int32 [B] on the device, codes in 0..7 (gdlhip.scene: 1 = flip x, 2 = flip y, 4 = transpose; a code that
    transposes needs a square tile).  The values are read back and checked here, before anything is launched, unless
    ``check_codes`` is False (a caller whose codes come from ``gdlhip.scene.tta_codes``, which checks the same; the kernels mask
    the codes, so a bad one never addresses outside a tile)."""
    _need_cuda(xforms)
    if xforms.dtype != torch.int32 or xforms.dim() != 1 or not xforms.is_contiguous():
        raise ValueError(f"{op}: xforms must be a contiguous int32 [B] tensor of transform codes, got {xforms.dtype} {tuple(xforms.shape)}")
    if xforms.shape[0] != B:
        raise ValueError(f"{op}: {xforms.shape[0]} transform codes for {B} tiles")
    if check_codes:
        codes = xforms.cpu()
        if int(codes.min()) < 0 or int(codes.max()) > 7:
            raise ValueError(f"{op}: a transform code is in 0..7, got {int(codes.min())}..{int(codes.max())}")
        if tile[0] != tile[1] and bool((codes & 4).any()):
            raise ValueError(f"{op}: a transform code with bit 4 (transpose) needs a square tile, not {tile[0]} x {tile[1]}")


def scene_cut_d4(raster: Tensor, origins: Tensor, xforms: Tensor, tile: tuple[int, int], mean: Tensor, std: Tensor, image_min: int = 0,
                 image_max: int = 255, norm_min: float = 0.0, norm_max: float = 1.0, fill: int = 0, *, check_codes: bool = True) -> Tensor:
    """``scene_cut`` with a transform per tile: tile ``b`` is ``gdlhip.scene.d4_apply`` of the tile ``scene_cut`` cuts at
    ``origins[b]``, with the code ``xforms[b]`` (int32 [B] on the device), bit for bit (gdl_scene_cut_d4)."""
    if xforms is None:
        raise ValueError("scene_cut_d4: xforms must be a contiguous int32 [B] tensor of transform codes, got None")
    B, th, tw = _scene_cut_check("scene_cut_d4", raster, origins, xforms, tile, mean, std, image_min, image_max, fill, check_codes)
    Cc, H, W = raster.shape
    out = torch.empty((B, Cc, th, tw), device=raster.device, dtype=torch.float32)
    _lib.checked().gdl_scene_cut_d4(_p(raster), _RAW_KIND[raster.dtype], Cc, H, W, _p(origins), _p(xforms), B, th, tw, int(fill), _p(out),
                                    int(image_min), int(image_max), float(norm_min), float(norm_max), _p(_f32vec(mean, Cc, "mean")),
                                    _p(_f32vec(std, Cc, "std")), _stream())
    return out


def scene_blend_d4(probs: Tensor, origins: Tensor, xforms: Tensor, wy: Tensor, wx: Tensor, canvas: Tensor,
                   box: tuple[int, int, int, int] | None = None, *, check_codes: bool = True) -> Tensor:
    """``scene_blend`` of probabilities [B, K, th, tw] f32 that are in the transformed frame of their tiles (the model's answer
    to ``scene_cut_d4``): the canvas takes the inverse transform of tile ``b``, code ``xforms[b]``, the window stays in the canvas
    frame.  The canvas is ``scene_blend`` of the inverse-permuted probabilities, bit for bit (gdl_scene_blend_d4)."""
    if probs.dtype != torch.float32 or probs.dim() != 4 or not probs.is_contiguous():
        raise ValueError("scene_blend_d4: contiguous f32 probabilities [B, K, th, tw] expected")
    B, K, th, tw = probs.shape
    H, W, y0, y1, x0, x1 = _scene_blend_check("scene_blend_d4", probs, K, (th, tw), origins, wy, wx, canvas, box)
    _scene_xforms("scene_blend_d4", xforms, B, (th, tw), check_codes)
    _lib.checked().gdl_scene_blend_d4(_p(probs), B, K, th, tw, _p(origins), _p(xforms), _p(wy), _p(wx), _p(canvas), H, W, y0, y1, x0, x1,
                                      _stream())
    return canvas


def scene_blend_lowres_d4(low: Tensor, size: tuple[int, int], origins: Tensor, xforms: Tensor, wy: Tensor, wx: Tensor, canvas: Tensor,
                          box: tuple[int, int, int, int] | None = None, *, check_codes: bool = True) -> Tensor:
    """``scene_blend_d4`` of ``upsample_probs(low, size)`` without those probabilities: ``low`` [B, h, w, K] is the head's NHWC
    f32 map of the transformed tile, evaluated where each canvas pixel lies in that tile (gdl_scene_blend_lowres_d4)."""
    if low.dtype != torch.float32 or low.dim() != 4 or not low.is_contiguous():
        raise ValueError("scene_blend_lowres_d4: contiguous f32 NHWC logits [B, h, w, K] expected")
    B, hi, wi, K = low.shape
    th, tw = int(size[0]), int(size[1])
    if min(hi, wi, th, tw) < 1:
        raise ValueError(f"scene_blend_lowres_d4: bad sizes {tuple(low.shape)} -> {th} x {tw}")
    H, W, y0, y1, x0, x1 = _scene_blend_check("scene_blend_lowres_d4", low, K, (th, tw), origins, wy, wx, canvas, box)
    _scene_xforms("scene_blend_lowres_d4", xforms, B, (th, tw), check_codes)
    _lib.checked().gdl_scene_blend_lowres_d4(_p(low), B, hi, wi, K, th, tw, _p(origins), _p(xforms), _p(wy), _p(wx), _p(canvas), H, W,
                                             y0, y1, x0, x1, _stream())
    return canvas


def scene_finish(canvas: Tensor, threshold: float = 0.5, return_probs: bool = False) -> tuple[Tensor, Tensor | None]:
    """Canvas [K+1, H, W] f32 -> (mask uint8 [H, W], probabilities f32 [K, H, W] or None): arg-max over the K weighted sums (the
    lowest index wins a tie) or, for one class, ``canvas[0] / canvas[1] > threshold``; a pixel that no tile covered (weight 0)
    gets mask 0 and probabilities 0 (gdl_scene_finish)."""
    _need_cuda(canvas)
    if canvas.dtype != torch.float32 or canvas.dim() != 3 or not canvas.is_contiguous() or not 2 <= canvas.shape[0] <= 17:
        raise ValueError(f"scene_finish: contiguous f32 canvas [K+1, H, W] with 1..16 classes expected, got {canvas.dtype} {tuple(canvas.shape)}")
    K, H, W = canvas.shape[0] - 1, int(canvas.shape[1]), int(canvas.shape[2])
    if H * W < 1:
        raise ValueError(f"scene_finish: empty canvas {tuple(canvas.shape)}")
    mask = torch.empty((H, W), device=canvas.device, dtype=torch.uint8)
    probs = torch.empty((K, H, W), device=canvas.device, dtype=torch.float32) if return_probs else None
    _lib.checked().gdl_scene_finish(_p(canvas), K, H * W, float(threshold), _p(mask), _p(probs), _stream())
    return mask, probs


# nodata (include/gdlhip_scene_nodata.h): a validity plane of the raster, its count per tile, and the cut and the labelling with it
NODATA_RULES = {"all": 0, "any": 1}


def scene_nodata_values(nodata, dtype: torch.dtype, channels: int, who: str = "scene_valid") -> Tensor:
    """The nodata value of every band as a host f32 [channels] vector, from one number or one per band.  A value that no sample of
    ``dtype`` can hold (a fraction, a NaN or a value outside the range of an integer raster) is a ValueError: it would never match,
    which is a mistake of the caller's and not a scene without nodata.  For an f32 raster every value goes, NaN included (a NaN
    sample is then nodata); it is compared after rounding to f32, as the samples were."""
    if isinstance(nodata, Tensor):
        nodata = nodata.detach().cpu().tolist()
    values = list(nodata) if isinstance(nodata, (list, tuple)) else [nodata]
    if any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in values) or not values:
        raise ValueError(f"{who}: nodata must be one number or one per band, got {nodata!r}")
    if len(values) == 1:
        values = values * int(channels)
    if len(values) != int(channels):
        raise ValueError(f"{who}: {len(values)} nodata values for {int(channels)} bands")
    if dtype in _RAW_LIMITS:
        lo, hi = _RAW_LIMITS[dtype]
        for v in values:
            if v != v:
                raise ValueError(f"{who}: a NaN nodata needs a float32 raster, not {dtype}")
            if abs(v) == float("inf") or v != int(v):
                raise ValueError(f"{who}: nodata {v!r} is not an integer, so no sample of {dtype} equals it")
            if not lo <= int(v) <= hi:
                raise ValueError(f"{who}: nodata {v!r} is outside {lo}..{hi}, so no sample of {dtype} equals it")
    elif dtype != torch.float32:
        raise ValueError(f"{who}: uint8/uint16/int16/float32 raster expected, got {dtype}")
    return torch.tensor([float(v) for v in values], dtype=torch.float64).float()


def _scene_plane(op: str, valid: Tensor, H: int, W: int) -> Tensor:
    """The plane as the kernels read it: uint8 (a bool plane is the same bytes) [H, W], contiguous, on the device."""
    _need_cuda(valid)
    if valid.dtype not in (torch.uint8, torch.bool) or tuple(valid.shape) != (H, W) or not valid.is_contiguous():
        raise ValueError(f"{op}: valid must be a contiguous uint8 / bool [H, W] = [{H}, {W}] plane, got {valid.dtype} {tuple(valid.shape)}")
    return valid.view(torch.uint8)


def scene_valid(raster: Tensor, nodata, rule: str = "all") -> Tensor:
    """uint8 [H, W], 1 where the raw raster [C, H, W] holds data: a sample is nodata when it equals its band's ``nodata`` (one
    number or one per band; NaN for an f32 raster: when it is NaN), and a pixel is invalid when every band (``rule="all"``, the
    dataset-mask convention) or at least one band (``"any"``) is nodata (gdl_scene_valid)."""
    if raster.dtype not in _RAW_KIND or not raster.is_contiguous() or raster.dim() != 3:
        raise ValueError(f"scene_valid: contiguous [C, H, W] uint8/uint16/int16/float32 raster expected, got {raster.dtype} {tuple(raster.shape)}")
    if rule not in NODATA_RULES:
        raise ValueError(f"scene_valid: unknown rule {rule!r} ('all' or 'any')")
    Cc, H, W = raster.shape
    values = scene_nodata_values(nodata, raster.dtype, Cc)
    _need_cuda(raster)
    if H * W < 1:
        raise ValueError(f"scene_valid: empty raster {tuple(raster.shape)}")
    valid = torch.empty((H, W), device=raster.device, dtype=torch.uint8)
    _lib.checked().gdl_scene_valid(_p(raster), _RAW_KIND[raster.dtype], Cc, H, W, _p(values.to(raster.device)), NODATA_RULES[rule],
                                   _p(valid), _stream())
    return valid


def scene_tile_valid(valid: Tensor, origins: Tensor, tile: tuple[int, int]) -> Tensor:
    """int32 [T] on the device: the number of valid pixels of each tile at ``origins`` (int32 [T, 2]) that lie inside the plane
    ``valid`` uint8 / bool [H, W]; origins may be negative or reach past it (gdl_scene_tile_valid)."""
    if valid.dim() != 2:
        raise ValueError(f"scene_tile_valid: valid must be a [H, W] plane, got {tuple(valid.shape)}")
    H, W = int(valid.shape[0]), int(valid.shape[1])
    plane = _scene_plane("scene_tile_valid", valid, H, W)
    _need_cuda(origins)
    T = _scene_origins("scene_tile_valid", origins)
    th, tw = int(tile[0]), int(tile[1])
    if th < 1 or tw < 1 or H * W < 1:
        raise ValueError(f"scene_tile_valid: bad sizes: tile {th} x {tw}, plane {H} x {W}")
    counts = torch.empty((T,), device=valid.device, dtype=torch.int32)
    _lib.checked().gdl_scene_tile_valid(_p(plane), H, W, _p(origins), T, th, tw, _p(counts), _stream())
    return counts


def scene_cut_valid(raster: Tensor, valid: Tensor, origins: Tensor, xforms: Tensor | None, tile: tuple[int, int], mean: Tensor,
                    std: Tensor, image_min: int = 0, image_max: int = 255, norm_min: float = 0.0, norm_max: float = 1.0, fill: int = 0,
                    *, check_codes: bool = True) -> Tensor:
    """``scene_cut`` (``xforms`` None) or ``scene_cut_d4`` in which a pixel whose ``valid`` (uint8 / bool [H, W]) is 0 takes the raw
    value ``fill``, like a position outside the raster.  With a plane of ones: their tiles, bit for bit (gdl_scene_cut_valid)."""
    B, th, tw = _scene_cut_check("scene_cut_valid", raster, origins, xforms, tile, mean, std, image_min, image_max, fill, check_codes)
    Cc, H, W = raster.shape
    plane = _scene_plane("scene_cut_valid", valid, H, W)
    out = torch.empty((B, Cc, th, tw), device=raster.device, dtype=torch.float32)
    _lib.checked().gdl_scene_cut_valid(_p(raster), _RAW_KIND[raster.dtype], Cc, H, W, _p(plane), _p(origins), _p(xforms), B, th, tw,
                                       int(fill), _p(out), int(image_min), int(image_max), float(norm_min), float(norm_max),
                                       _p(_f32vec(mean, Cc, "mean")), _p(_f32vec(std, Cc, "std")), _stream())
    return out


def scene_finish_valid(canvas: Tensor, valid: Tensor | None, nodata_label: int = 255, threshold: float = 0.5,
                       return_probs: bool = False) -> tuple[Tensor, Tensor | None]:
    """``scene_finish`` in which a pixel whose ``valid`` (uint8 / bool [H, W], or None) is 0 or that no tile covered gets the mask
    ``nodata_label`` (0..255) and probabilities 0; every other pixel gets the bits of ``scene_finish`` (gdl_scene_finish_valid)."""
    _need_cuda(canvas)
    if canvas.dtype != torch.float32 or canvas.dim() != 3 or not canvas.is_contiguous() or not 2 <= canvas.shape[0] <= 17:
        raise ValueError(f"scene_finish_valid: contiguous f32 canvas [K+1, H, W] with 1..16 classes expected, got {canvas.dtype} {tuple(canvas.shape)}")
    byte_check("scene_finish_valid", "nodata_label", nodata_label)
    K, H, W = canvas.shape[0] - 1, int(canvas.shape[1]), int(canvas.shape[2])
    if H * W < 1:
        raise ValueError(f"scene_finish_valid: empty canvas {tuple(canvas.shape)}")
    plane = None if valid is None else _scene_plane("scene_finish_valid", valid, H, W)
    mask = torch.empty((H, W), device=canvas.device, dtype=torch.uint8)
    probs = torch.empty((K, H, W), device=canvas.device, dtype=torch.float32) if return_probs else None
    _lib.checked().gdl_scene_finish_valid(_p(canvas), K, H * W, float(threshold), _p(plane), nodata_label, _p(mask), _p(probs), _stream())
    return mask, probs


# what the vector stages below share: the range of a mask value, the labels argument and the scratch of a scan
def is_byte(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, int) and 0 <= v <= 255


def byte_check(who: str, name: str, v, none_ok: bool = False) -> None:
    """ValueError unless ``v`` is an int in 0..255 (a mask value), or None where ``none_ok``."""
    if not (is_byte(v) or (none_ok and v is None)):
        raise ValueError(f"{who}: {name} must be {'None or ' if none_ok else ''}an int in 0..255, got {v!r}")


def _labels_check(op: str, labels, H: int, W: int) -> None:
    if labels is not None and (not isinstance(labels, Tensor) or labels.dtype != torch.int32 or tuple(labels.shape) != (H, W)
                               or not labels.is_contiguous()):
        got = f"{labels.dtype} {tuple(labels.shape)}" if isinstance(labels, Tensor) else type(labels).__name__
        raise ValueError(f"{op}: labels must be a contiguous int32 [H, W] = [{H}, {W}] tensor, got {got}")


def _i32(dev, n: int) -> Tensor:
    return torch.empty((n,), device=dev, dtype=torch.int32)


def _scan_blocks(n: int, tile: int) -> int:
    """The block sums a scan over n entries needs (tile: the stage's GDL_SCENE_*_SCAN_TILE)."""
    return -(-n // tile)


# the sieve (include/gdlhip_scene_sieve.h): connected components of a label mask, the small ones dissolved into their neighbours
def _sieve_check(op: str, mask: Tensor, connectivity: int, ignore_label: int | None) -> tuple[Tensor, int, int, int]:
    """The argument checks the two calls share, but for the device (which is asked for last); (the mask as uint8, H, W,
    ignore_label or -1)."""
    if not isinstance(mask, Tensor) or mask.dtype not in (torch.uint8, torch.bool) or mask.dim() != 2 or not mask.is_contiguous():
        got = f"{mask.dtype} {tuple(mask.shape)}" if isinstance(mask, Tensor) else type(mask).__name__
        raise ValueError(f"{op}: contiguous uint8 / bool [H, W] mask expected, got {got}")
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"{op}: connectivity must be 4 or 8, got {connectivity!r}")
    byte_check(op, "ignore_label", ignore_label, none_ok=True)
    H, W = int(mask.shape[0]), int(mask.shape[1])
    if H * W < 1:
        raise ValueError(f"{op}: empty mask {tuple(mask.shape)}")
    if H * W >= 2 ** 31:
        raise ValueError(f"{op}: {H} x {W} pixels: a linear index must fit an int32 (H * W < 2^31)")
    return mask.view(torch.uint8), H, W, -1 if ignore_label is None else ignore_label


def scene_components(mask: Tensor, connectivity: int = 4, ignore_label: int | None = None) -> tuple[Tensor, Tensor]:
    """(labels int32 [H, W], sizes int32 [H*W]) of a uint8 / bool mask [H, W] on the device.  A component is a maximal set of equal
    pixels connected under ``connectivity`` (4 or 8); ``labels`` holds the smallest linear index ``y * W + x`` of the pixel's
    component and ``sizes`` the pixel count of a component at that index, 0 elsewhere.  Pixels equal to ``ignore_label`` belong to
    no component: label -1.  Exact and the same bits from run to run (gdl_scene_components)."""
    m, H, W, ignore = _sieve_check("scene_components", mask, connectivity, ignore_label)
    _need_cuda(mask)
    labels = torch.empty((H, W), device=mask.device, dtype=torch.int32)
    sizes = torch.empty((H * W,), device=mask.device, dtype=torch.int32)
    _lib.checked().gdl_scene_components(_p(m), H, W, connectivity, ignore, _p(labels), _p(sizes), _stream())
    return labels, sizes


def scene_sieve(mask: Tensor, min_size: int, connectivity: int = 4, ignore_label: int | None = None, iterations: int = 1) -> Tensor:
    """A new uint8 [H, W] mask in which every component of fewer than ``min_size`` pixels has taken the value of the largest
    component of at least ``min_size`` pixels that touches it (of two equally large ones: the lower value); one that touches none
    keeps its value, and so does every pixel equal to ``ignore_label``.  ``iterations`` repeats labelling and sieving on the
    result, which lets a small component surrounded by small ones go once those have gone.  ``min_size <= 1`` copies the mask
    (gdl_scene_components + gdl_scene_sieve)."""
    m, H, W, ignore = _sieve_check("scene_sieve", mask, connectivity, ignore_label)
    if isinstance(min_size, bool) or not isinstance(min_size, int):
        raise ValueError(f"scene_sieve: min_size must be an int (a pixel count), got {min_size!r}")
    if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
        raise ValueError(f"scene_sieve: iterations must be an int of at least 1, got {iterations!r}")
    _need_cuda(mask)
    if min_size <= 1:
        return m.clone()
    min_size = min(min_size, 2 ** 31 - 1)      # no component has more pixels than that
    labels = torch.empty((H, W), device=mask.device, dtype=torch.int32)
    sizes = torch.empty((H * W,), device=mask.device, dtype=torch.int32)
    best = torch.empty((H * W,), device=mask.device, dtype=torch.int64)
    lib, src = _lib.checked(), m
    for _ in range(iterations):
        out = torch.empty_like(m)
        lib.gdl_scene_components(_p(src), H, W, connectivity, ignore, _p(labels), _p(sizes), _stream())
        lib.gdl_scene_sieve(_p(src), _p(labels), _p(sizes), H, W, connectivity, min_size, ignore, _p(best), _p(out), _stream())
        src = out
    return src


# the polygon rings (include/gdlhip_scene_rings.h): the boundaries of a mask's regions as closed rings of lattice points
class SceneRings(NamedTuple):
    vertices: Tensor          # int32 [V, 2]: (x, y) lattice points, ring after ring, every ring open
    ring_offsets: Tensor      # int32 [R + 1]: ring r is vertices[ring_offsets[r]:ring_offsets[r + 1]]
    value: Tensor             # uint8 [R]: the class of the ring's pixels
    label: Tensor             # int32 [R]: their component (scene_components)
    start: Tensor             # int32 [R]: the ring's smallest slot 4 * (y * W + x) + side, ascending
    area2: Tensor             # int64 [R]: twice the enclosed pixel count for an exterior ring, negative for a hole


def _keep_table(values) -> list[int]:
    """256 flags of the keep set ``values`` (None: every value)."""
    if values is None:
        return [1] * 256
    items = None if isinstance(values, (str, bytes, Tensor)) or not hasattr(values, "__iter__") else list(values)
    if items is None or not all(is_byte(v) for v in items):
        raise ValueError(f"scene_rings: values must be None or an iterable of ints in 0..255, got {values!r}")
    return [int(v in items) for v in range(256)]


def scene_rings(mask: Tensor, connectivity: int = 4, ignore_label: int | None = None, values=None,
                labels: Tensor | None = None) -> SceneRings:
    """The boundaries of the regions of a uint8 / bool mask [H, W] on the device as closed rings of lattice points (pixel (y, x)
    is the square (x, y) .. (x + 1, y + 1)), the region on the right hand of the direction of travel: an exterior ring has
    ``area2 > 0``, a hole ``area2 < 0``.  A region is a component of ``scene_components`` under ``connectivity`` and
    ``ignore_label``; ``values`` (an iterable of ints in 0..255) keeps the regions of those classes alone.  ``labels``: the int32
    [H, W] labels ``scene_components`` gave for the same mask, connectivity and ignore_label, computed here when None.  Rings
    start at their smallest slot and come in the order of their starts; every component has one exterior ring, whose start is
    ``4 * label``.  Exact and the same bits from run to run; the mask is not modified.  Two small device-to-host copies (the
    number of boundary sides, then of rings and vertices) size the buffers (gdl_scene_rings_count / _trace / _write)."""
    m, H, W, ignore = _sieve_check("scene_rings", mask, connectivity, ignore_label)
    if H * W >= 2 ** 29:
        raise ValueError(f"scene_rings: {H} x {W} pixels: a slot 4 * (y * W + x) + side must fit an int32 (H * W < 2^29)")
    table = _keep_table(values)
    _labels_check("scene_rings", labels, H, W)
    _need_cuda(mask, labels)
    dev, lib, tile = mask.device, _lib.checked(), _lib.SCENE_RINGS_SCAN_TILE
    if labels is None:
        labels = scene_components(m, connectivity, ignore_label)[0]
    keep = torch.tensor(table, dtype=torch.uint8).to(dev)
    offsets, n_sides = _i32(dev, H * W), _i32(dev, 1)
    lib.gdl_scene_rings_count(_p(m), H, W, ignore, _p(keep), _p(offsets), _p(_i32(dev, _scan_blocks(H * W, tile))), _p(n_sides), _stream())
    E = int(n_sides.item())
    side_slot, side_next, side_ring, side_rank = (_i32(dev, E) for _ in range(4))
    work, counts = _i32(dev, 3 * E + 2 * _scan_blocks(E, tile) + _lib.SCENE_RINGS_FLAGS), _i32(dev, 2)
    lib.gdl_scene_rings_trace(_p(m), H, W, connectivity, ignore, _p(keep), _p(offsets), E, _p(side_slot), _p(side_next), _p(side_ring),
                              _p(side_rank), _p(work), _p(counts), _stream())
    R, V = (int(c) for c in counts.tolist())
    out = SceneRings(torch.empty((V, 2), device=dev, dtype=torch.int32), _i32(dev, R + 1), torch.empty((R,), device=dev, dtype=torch.uint8),
                     _i32(dev, R), _i32(dev, R), torch.empty((R,), device=dev, dtype=torch.int64))
    lib.gdl_scene_rings_write(_p(m), _p(labels), W, E, R, V, _p(side_slot), _p(side_next), _p(side_ring), _p(side_rank), _p(work),
                              *(_p(t) for t in out), _stream())
    return out


# their simplification (include/gdlhip_scene_simplify.h): Douglas-Peucker per arc between the junctions of the boundaries
SIMPLIFY_TOLERANCE_MAX = 2 ** 20      # pixels; tol_q8 = round(tolerance * 256) then fits 2^28


def simplify_tolerance_ok(x) -> bool:
    """Whether ``x`` is a tolerance ``scene_rings_simplify`` takes: a finite number of pixels in 0..SIMPLIFY_TOLERANCE_MAX."""
    return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x) and 0 <= x <= SIMPLIFY_TOLERANCE_MAX


_RING_FIELDS = {"vertices": torch.int32, "ring_offsets": torch.int32, "value": torch.uint8, "label": torch.int32, "start": torch.int32,
                "area2": torch.int64}      # of SceneRings, in its order


def _ring_fields_check(op: str, rings, names: tuple, must_have: str) -> tuple[int, int]:
    """(R, V) of rings whose fields ``names`` (vertices and ring_offsets first) belong together by type, shape and device, or
    ValueError; ``must_have``: how the message calls the fields."""
    got = [getattr(rings, name, None) for name in names]
    if not all(isinstance(t, Tensor) for t in got):
        raise ValueError(f"{op}: rings must have {must_have}, got {type(rings).__name__}")
    vertices, offsets = got[0], got[1]
    R = int(offsets.numel()) - 1
    shapes = {"vertices": (int(vertices.shape[0]), 2) if vertices.dim() else None, "ring_offsets": (R + 1,)}
    for name, t in zip(names, got):
        dtype, shape = _RING_FIELDS[name], shapes.get(name, (R,))
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != vertices.device:
            raise ValueError(f"{op}: rings.{name} must be a contiguous {dtype} {shape} tensor on {vertices.device}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
    return R, int(vertices.shape[0])


def _rings_check(op: str, rings) -> tuple[int, int]:
    """(R, V) of a SceneRings whose six fields belong together by type, shape and device, or ValueError."""
    names = tuple(_RING_FIELDS)
    R, V = _ring_fields_check(op, rings, names, f"the six tensor fields of SceneRings ({', '.join(names)})")
    if R < 0 or 4 * R > V or (R == 0) != (V == 0):
        raise ValueError(f"{op}: {R} rings and {V} vertices do not belong together (a ring has at least 4 vertices)")
    return R, V


def scene_rings_simplify(rings: SceneRings, mask: Tensor, tolerance: float, ignore_label: int | None = None, values=None) -> SceneRings:
    """The rings of ``scene_rings`` simplified by Douglas-Peucker with ``tolerance`` (pixels, 0 .. 2^20, quantised to 1 / 256),
    arc by arc between the nodes of the boundaries -- the lattice points where three or four boundary edges meet -- so that two
    regions that share a boundary get the same simplified boundary, vertex for vertex, and no gap or overlap opens between them.
    ``mask``, ``ignore_label`` and ``values`` must be those ``rings`` was made with: they define the nodes.  The result has the
    same rings in the same order; ``value``, ``label``, ``start`` and ``area2`` are the input's tensors, so ``area2`` stays the
    area of the *pixel* ring (``gdlhip.scene.polygons`` still tells exterior from hole by it, and its ``pixels`` stays the true
    pixel count).  Nodes are always kept, also where a ring runs straight through one; a ring without nodes (an island, a hole
    between two regions) keeps its smallest (y, x) vertex.  A ring may come out with fewer than 3 vertices: it collapsed.
    ``tolerance=0`` drops the vertices at distance 0 from their chords alone.  Integer arithmetic: exact, and the same bits from
    run to run; neither the rings nor the mask are modified.  Small device-to-host copies size the buffers and end the rounds:
    the dense vertex count, one flag per group of ``GDL_SCENE_SIMPLIFY_ROUNDS`` rounds (the depth of Douglas-Peucker depends
    on the data), and the output vertex count (gdl_scene_nodes / gdl_scene_simplify_count / _dense / _rounds / _write)."""
    op = "scene_rings_simplify"
    if not simplify_tolerance_ok(tolerance):
        raise ValueError(f"{op}: tolerance must be a finite number of pixels in 0..2^20, got {tolerance!r}")
    R, V = _rings_check(op, rings)
    m, H, W, ignore = _sieve_check(op, mask, 4, ignore_label)
    if H * W >= 2 ** 29:
        raise ValueError(f"{op}: {H} x {W} pixels: the rings are those of a raster of H * W < 2^29")
    if V > 4 * H * W:
        raise ValueError(f"{op}: {V} vertices are more than a {H} x {W} mask has pixel sides")
    table = _keep_table(values)
    if rings.vertices.device != mask.device:
        raise ValueError(f"{op}: the rings are on {rings.vertices.device}, the mask on {mask.device}")
    _need_cuda(mask, rings.vertices)
    dev, lib, tol_q8, tile = mask.device, _lib.checked(), int(round(tolerance * 256)), _lib.SCENE_SIMPLIFY_SCAN_TILE
    if R == 0:
        return SceneRings(torch.empty((0, 2), device=dev, dtype=torch.int32), torch.zeros((1,), device=dev, dtype=torch.int32), rings.value, rings.label, rings.start, rings.area2)
    keep = torch.tensor(table, dtype=torch.uint8).to(dev)
    nodes = torch.empty((H + 1, W + 1), device=dev, dtype=torch.uint8)
    lib.gdl_scene_nodes(_p(m), H, W, ignore, _p(keep), _p(nodes), _stream())
    pos, n_dense = _i32(dev, V + 1), _i32(dev, 1)
    lib.gdl_scene_simplify_count(_p(nodes), H, W, _p(rings.vertices), _p(rings.ring_offsets), R, V, _p(pos),
                                 _p(_i32(dev, _scan_blocks(V + 1, tile))), _p(n_dense), _stream())
    D = int(n_dense.item())
    dense, dense_offsets = torch.empty((D, 2), device=dev, dtype=torch.int32), _i32(dev, R + 1)
    kept, seg = torch.empty((D,), device=dev, dtype=torch.uint8), _i32(dev, 4 * D + _lib.SCENE_SIMPLIFY_ROUNDS)
    key = torch.empty((D,), device=dev, dtype=torch.int64)
    work = torch.empty((R + D + 1 + _scan_blocks(D + 1, tile),), device=dev, dtype=torch.int64)      # int64: 8-byte aligned, at least as large
    lib.gdl_scene_simplify_dense(_p(nodes), H, W, _p(rings.vertices), _p(rings.ring_offsets), R, V, _p(pos), D, _p(dense),
                                 _p(dense_offsets), _p(kept), _p(seg), _p(key), _p(work), _stream())
    del work, pos, nodes
    changed, first = _i32(dev, 1), 1
    while True:
        lib.gdl_scene_simplify_rounds(_p(dense), W, D, tol_q8, first, _lib.SCENE_SIMPLIFY_ROUNDS, _p(kept), _p(seg), _p(key), _p(changed),
                                      _stream())
        first = 0
        if not int(changed.item()):
            break
    del seg, key
    out, offsets, n_out = torch.empty((D, 2), device=dev, dtype=torch.int32), _i32(dev, R + 1), _i32(dev, 1)
    lib.gdl_scene_simplify_write(_p(dense), _p(dense_offsets), R, D, _p(kept), _p(_i32(dev, D + 1 + _scan_blocks(D + 1, tile))), _p(out),
                                 _p(offsets), _p(n_out), _stream())
    n = int(n_out.item())
    return SceneRings(out if n == D else out[:n].clone(), offsets, rings.value, rings.label, rings.start, rings.area2)


# the per-region attributes (include/gdlhip_scene_regions.h): what a vector layer says about each polygon
class SceneRegions(NamedTuple):
    label: Tensor             # int32 [N]: the region's label (scene_components), ascending
    value: Tensor             # uint8 [N]: the class of its pixels
    pixels: Tensor            # int32 [N]: their number
    bbox: Tensor              # int32 [N, 4]: (x0, y0, x1, y1) in pixel indices, x1 and y1 exclusive
    sum_xy: Tensor            # int64 [N, 2]: the sums of the pixels' x and of their y
    conf_sum: Tensor | None   # int64 [N]: the sum of the pixels' confidence q (0 .. 65536 each); None without a canvas
    conf_min: Tensor | None   # int32 [N]: the smallest q of the region; None without a canvas


def scene_regions(mask: Tensor, connectivity: int = 4, ignore_label: int | None = None, canvas: Tensor | None = None,
                  labels: Tensor | None = None) -> SceneRegions:
    """The attributes of every region of a uint8 / bool mask [H, W] on the device: one entry per component of
    ``scene_components`` under ``connectivity`` and ``ignore_label``, in the order of the labels.  ``labels``: the int32 [H, W]
    labels ``scene_components`` gave for the same mask, connectivity and ignore_label, computed here when None.  ``canvas``: the
    contiguous f32 [K + 1, H, W] canvas the mask was labelled from (``SceneInference.canvas``), on the mask's device; with it a
    pixel of class v has the confidence ``q = rint(65536 * canvas[v] / canvas[K])`` (one class: ``1 - canvas[0] / canvas[K]``
    where v is 0), the quotient being the very expression ``scene_finish`` writes to ``probs``; q is 0 where the weight is 0 or
    the canvas has no plane for v.  ``conf_sum / (65536 * pixels)`` is the region's mean confidence, ``conf_min / 65536`` its
    lowest.  Integer sums, minima and maxima alone: exact and the same bits from run to run; no input is modified.  One small
    device-to-host copy (the number of regions) sizes the arrays; a mask of ignored pixels alone gives empty ones
    (gdl_scene_regions_count / _stats)."""
    op = "scene_regions"
    m, H, W, ignore = _sieve_check(op, mask, connectivity, ignore_label)
    _labels_check(op, labels, H, W)
    K = 0
    if canvas is not None:
        if not isinstance(canvas, Tensor) or canvas.dtype != torch.float32 or canvas.dim() != 3 or tuple(canvas.shape[1:]) != (H, W) \
                or not 2 <= canvas.shape[0] <= 256 or not canvas.is_contiguous():
            got = f"{canvas.dtype} {tuple(canvas.shape)}" if isinstance(canvas, Tensor) else type(canvas).__name__
            raise ValueError(f"{op}: canvas must be a contiguous f32 [K + 1, H, W] = [2..256, {H}, {W}] tensor, got {got}")
        if canvas.device != mask.device:
            raise ValueError(f"{op}: the canvas is on {canvas.device}, the mask on {mask.device}")
        K = int(canvas.shape[0]) - 1
    if labels is not None and labels.device != mask.device:
        raise ValueError(f"{op}: the labels are on {labels.device}, the mask on {mask.device}")
    _need_cuda(mask, labels, canvas)
    dev, lib = mask.device, _lib.checked()
    if labels is None:
        labels = scene_components(m, connectivity, ignore_label)[0]

    def new(shape: tuple, dtype: torch.dtype) -> Tensor:
        return torch.empty(shape, device=dev, dtype=dtype)

    rank, n_regions = new((H * W,), torch.int32), new((1,), torch.int32)
    bsum = _i32(dev, _scan_blocks(H * W, _lib.SCENE_REGIONS_SCAN_TILE))
    lib.gdl_scene_regions_count(_p(labels), H, W, _p(rank), _p(bsum), _p(n_regions), _stream())
    N = int(n_regions.item())
    conf = canvas is not None
    out = SceneRegions(new((N,), torch.int32), new((N,), torch.uint8), new((N,), torch.int32), new((N, 4), torch.int32),
                       new((N, 2), torch.int64), new((N,), torch.int64) if conf else None, new((N,), torch.int32) if conf else None)
    if N > 0:
        lib.gdl_scene_regions_stats(_p(m), _p(labels), _p(rank), _p(canvas), K, H, W, N, *(_p(t) for t in out), _stream())
    return out


# rings burned into a raster (include/gdlhip_scene_burn.h): the inverse of scene_rings
class SceneBurn(NamedTuple):
    mask: Tensor              # uint8 [H, W]: the ring's value inside a ring, `background` outside all, `conflict` elsewhere
    conflicts: int            # the pixels that are neither: overlaps, crossed arcs, reversed rings
    differ: int | None        # the pixels where mask != reference; None without a reference


def _burn_check(op: str, rings, size, bits, background, conflict, reference) -> tuple[int, int, int, int]:
    """The argument checks of ``scene_burn`` but for the device (which is asked for last); (R, V, H, W)."""
    names = ("vertices", "ring_offsets", "value")
    R, V = _ring_fields_check(op, rings, names, f"the tensor fields {', '.join(names)}")
    vertices = rings.vertices
    if R < 0:
        raise ValueError(f"{op}: rings.ring_offsets must hold R + 1 >= 1 offsets, got none")
    try:
        H, W = size
        ok = all(isinstance(n, int) and not isinstance(n, bool) for n in (H, W))
    except (TypeError, ValueError):
        ok = False
    if not ok or H < 1 or W < 1:
        raise ValueError(f"{op}: size must be (H, W), two ints of at least 1, got {size!r}")
    if H * W >= 2 ** 31:
        raise ValueError(f"{op}: {H} x {W} pixels: a linear index must fit an int32 (H * W < 2^31)")
    if isinstance(bits, bool) or not isinstance(bits, int) or not 0 <= bits <= _lib.SCENE_BURN_BITS_MAX:
        raise ValueError(f"{op}: bits must be an int in 0..{_lib.SCENE_BURN_BITS_MAX}, got {bits!r}")
    byte_check(op, "background", background)
    byte_check(op, "conflict", conflict)
    if reference is not None:
        if not isinstance(reference, Tensor) or reference.dtype not in (torch.uint8, torch.bool) or tuple(reference.shape) != (H, W) \
                or not reference.is_contiguous():
            what = f"{reference.dtype} {tuple(reference.shape)}" if isinstance(reference, Tensor) else type(reference).__name__
            raise ValueError(f"{op}: reference must be a contiguous uint8 / bool [H, W] = [{H}, {W}] tensor, got {what}")
        if reference.device != vertices.device:
            raise ValueError(f"{op}: the reference is on {reference.device}, the rings on {vertices.device}")
    return R, V, H, W


def scene_burn(rings, size: tuple[int, int], *, bits: int = 0, background: int = 0, conflict: int = 255,
               reference: Tensor | None = None) -> SceneBurn:
    """Polygon rings burned into a uint8 raster of ``size`` = (H, W): the inverse of ``scene_rings``, what GDAL rasterize does.
    ``rings``: a ``SceneRings`` or anything with ``vertices`` (int32 [V, 2] of (x, y)), ``ring_offsets`` (int32 [R + 1]) and
    ``value`` (uint8 [R]) on the device; rings are open, have their region on the right hand (an exterior ring has a positive
    shoelace sum with y down, a hole a negative one), and one of fewer than 3 vertices contributes nothing.  Coordinates are in
    units of 1 / 2^``bits`` pixel (``bits`` 0..8; 0 is the lattice of ``scene_rings`` and ``scene_rings_simplify``), at most
    2^20 pixels in magnitude, and may lie outside the raster.  A pixel belongs to a ring when its centre lies inside, a centre
    exactly on an edge counting as right of it for every ring alike, so rings that share an edge share no pixel.  The pixel is
    the ring's ``value`` where exactly one region covers it, ``background`` where none does (a hole whose island is missing
    included) and ``conflict`` everywhere else; ``conflicts`` counts the last kind.  ``reference``: a uint8 / bool [H, W]
    plane on the device; ``differ`` is then the number of pixels where the result is not the reference.  Integer sums alone:
    exact, independent of the order of the rings, and the same bits from run to run; the rings are not modified.  Two small
    device-to-host copies: the number of crossings and of bad entries, then the two counts (gdl_scene_burn_count / _fill).
    A coordinate out of range, offsets that do not ascend inside 0..V, and 2^31 or more crossings are a ValueError."""
    op = "scene_burn"
    R, V, H, W = _burn_check(op, rings, size, bits, background, conflict, reference)
    _need_cuda(rings.vertices, reference)
    dev, lib = rings.vertices.device, _lib.checked()
    n_cross = 0
    edge_ring = edge_rows = plane = None
    if R > 0 and V > 0:
        edge_ring, edge_rows = _i32(dev, V), _i32(dev, V + 1)
        bsum = _i32(dev, _scan_blocks(V + 1, _lib.SCENE_BURN_SCAN_TILE))
        found = torch.empty((2,), device=dev, dtype=torch.int64)
        lib.gdl_scene_burn_count(_p(rings.vertices), _p(rings.ring_offsets), R, V, bits, H, W, _p(edge_ring), _p(edge_rows), _p(bsum),
                                 _p(found), _stream())
        n_cross, bad = (int(c) for c in found.tolist())
        if bad:
            raise ValueError(f"{op}: {bad} bad entries in the rings: a coordinate beyond 2^20 pixels, or ring_offsets that do not "
                             f"ascend inside 0..{V}")
        if n_cross >= 2 ** 31:
            raise ValueError(f"{op}: {n_cross} crossings of ring edges with raster rows: fewer than 2^31 are supported")
        if n_cross > 0:
            plane = torch.empty((2, H, W), device=dev, dtype=torch.int32)
    out, counts = torch.empty((H, W), device=dev, dtype=torch.uint8), torch.empty((2,), device=dev, dtype=torch.int64)
    ref = None if reference is None else reference.view(torch.uint8)
    lib.gdl_scene_burn_fill(_p(rings.vertices), _p(rings.ring_offsets), _p(rings.value), R, V, bits, H, W, _p(edge_ring), _p(edge_rows),
                            n_cross, background, conflict, _p(ref), _p(plane), _p(out), _p(counts), _stream())
    conflicts, differ = (int(c) for c in counts.tolist())
    return SceneBurn(out, conflicts, None if reference is None else differ)


def iou_counts(pred: Tensor, target: Tensor, num_classes: int) -> Tensor:
    """int64 [B, 3, K]: per sample and class (intersection, |pred==k|, |target==k|); exact integer counts."""
    _need_cuda(pred, target)
    if pred.dtype != torch.int64 or target.dtype != torch.int64 or pred.shape != target.shape:
        raise ValueError("iou_counts: int64 index tensors of one shape expected")
    B = pred.shape[0]
    p2, t2 = pred.reshape(B, -1).contiguous(), target.reshape(B, -1).contiguous()
    counts = torch.empty((B, 3, num_classes), device=pred.device, dtype=torch.int64)
    _lib.checked().gdl_iou_counts(_p(p2), _p(t2), B, p2.shape[1], num_classes, _p(counts), _stream())
    return counts


class DiceOptions(NamedTuple):
    """The constructor options of smp's DiceLoss that the gdl_dice_*_opt_* entry points take (gdl_dice_options in
    include/gdlhip.h): ``ignore_index`` (any int64, or None), ``smooth``, ``log_loss``, ``classes`` (a tuple of distinct class
    indices, or None for all)."""

    ignore_index: int | None = None
    smooth: float = 0.0
    log_loss: bool = False
    classes: tuple | None = None

    def c_arg(self):
        """(pointer for the C call, objects that must stay alive during it)"""
        arr = (C.c_int * len(self.classes))(*self.classes) if self.classes else None
        o = _lib.DiceOptions(int(self.ignore_index is not None), int(self.ignore_index or 0), float(self.smooth),
                             int(bool(self.log_loss)), C.cast(arr, C.POINTER(C.c_int)) if arr is not None else None,
                             len(self.classes) if self.classes else 0)
        return C.addressof(o), (o, arr)


class OverlapOptions(NamedTuple):
    """What the gdl_overlap_* entry points take (gdl_overlap_options in include/gdlhip.h): ``kind`` "jaccard" or "tversky", then
    ``ignore_index`` (any int64, or None; Tversky only), ``smooth``, ``log_loss``, ``classes`` as in DiceOptions, and Tversky's
    ``alpha``, ``beta``, ``gamma`` (not read for Jaccard)."""

    kind: str
    ignore_index: int | None = None
    smooth: float = 0.0
    log_loss: bool = False
    classes: tuple | None = None
    alpha: float = 0.5
    beta: float = 0.5
    gamma: float = 1.0

    def c_arg(self):
        """(pointer for the C call, objects that must stay alive during it)"""
        kind = {"jaccard": _lib.OVERLAP_JACCARD, "tversky": _lib.OVERLAP_TVERSKY}[self.kind]
        arr = (C.c_int * len(self.classes))(*self.classes) if self.classes else None
        o = _lib.OverlapOptions(kind, int(self.ignore_index is not None), int(self.ignore_index or 0), float(self.smooth),
                                int(bool(self.log_loss)), float(self.alpha), float(self.beta), float(self.gamma),
                                C.cast(arr, C.POINTER(C.c_int)) if arr is not None else None,
                                len(self.classes) if self.classes else 0)
        return C.addressof(o), (o, arr)


# the `form` argument of the low-resolution backwards that have two
LOWRES_BWD_FORMS = {"auto": _lib.FOCAL_AUTO, "gather": _lib.FOCAL_GATHER, "tile": _lib.FOCAL_TILE}
FOCAL_FORMS = LOWRES_BWD_FORMS      # (the name it had while FocalLoss was its only user)


def _logits_target_check(who: str, logits: Tensor, target: Tensor, want_target: tuple, layout: str) -> None:
    _need_cuda(logits, target)
    if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() != 4:
        raise ValueError(f"{who}: contiguous f32 {layout} logits expected")
    if target.dtype != torch.int64 or not target.is_contiguous() or tuple(target.shape) != want_target:
        raise ValueError(f"{who}: contiguous int64 target {list(want_target)} expected, got {tuple(target.shape)}")


def _nchw_check(who: str, logits: Tensor, target: Tensor) -> tuple:
    """(B, K, HW) of contiguous f32 NCHW logits [B, K, H, W] with a contiguous int64 target [B, H, W]."""
    B, K, H, W = logits.shape if logits.dim() == 4 else (0, 0, 0, 0)
    _logits_target_check(who, logits, target, (B, H, W), "NCHW")
    return B, K, H * W


def _lowres_check(who: str, low: Tensor, target: Tensor, size: tuple[int, int]) -> tuple:
    """``dims`` = (B, K, h, w, H, W), as the low-resolution entry points take them, of a contiguous f32 NHWC map [B, h, w, K] with a
    contiguous int64 target [B, H, W] at ``size``."""
    B, Hi, Wi, K = low.shape if low.dim() == 4 else (0, 0, 0, 0)
    dims = (B, K, Hi, Wi, int(size[0]), int(size[1]))
    _logits_target_check(who, low, target, (B, dims[4], dims[5]), "NHWC low-resolution [B, h, w, K]")
    return dims


def _loss_buffers(like: Tensor, nbytes: int, norm: bool = False):
    """(loss [], norm [1] or None, f64 workspace of ``nbytes``) for a forward, on ``like``'s device."""
    return (torch.empty((), device=like.device, dtype=torch.float32),
            torch.empty(1, device=like.device, dtype=torch.float32) if norm else None,
            torch.empty(nbytes // 8, device=like.device, dtype=torch.float64))


def _grad_out(who: str, logits: Tensor, out: Tensor | None) -> Tensor:
    """``out`` (the caller's buffer for a full-resolution gradient) checked, or a new one."""
    if out is None:
        return torch.empty_like(logits)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.shape != logits.shape:
        raise ValueError(f"{who}: out must be a contiguous f32 tensor of the logits' shape")
    return out


def _bwd_workspace(query, dims: tuple, like: Tensor, form: str = "auto"):
    """(f32 workspace or None, its bytes) of a low-resolution backward: what ``query(*dims)`` asks for -- only the tile kernels
    need one, so nothing with ``form`` "gather"."""
    nbytes = query(*dims) if form != "gather" else 0
    return (torch.empty(nbytes // 4, device=like.device, dtype=torch.float32) if nbytes else None), nbytes


def _dice_entry(stem: str, way: str, options):
    """The C entry point of the Dice / Jaccard / Tversky family for ``options``: (function of the checked view, the option arguments
    that follow ``eps`` in its signature, objects to keep alive during the call).  None: the plain ``gdl_dice_<stem>_<way>`` (no option
    argument); DiceOptions: ``gdl_dice_<stem>_opt_<way>``; OverlapOptions: ``gdl_overlap_<stem>_<way>``."""
    if options is None:
        name, opt, keep = f"gdl_dice_{stem}_{way}", (), None
    else:
        name = f"gdl_overlap_{stem}_{way}" if isinstance(options, OverlapOptions) else f"gdl_dice_{stem}_opt_{way}"
        addr, keep = options.c_arg()
        opt = (addr,)
    return getattr(_lib.checked(), name), opt, keep


def _dice_buffers(like: Tensor, K: int, nbytes: int):
    """(sums [3K], loss [], workspace of ``nbytes``) for a forward of the family, on ``like``'s device."""
    sums = torch.empty(3 * K, device=like.device, dtype=torch.float32)
    loss = torch.empty((), device=like.device, dtype=torch.float32)
    return sums, loss, torch.empty(nbytes // 4, device=like.device, dtype=torch.float32)


def dice_loss_fwd(logits: Tensor, target: Tensor, eps: float = 1e-7, options: DiceOptions | OverlapOptions | None = None):
    """(loss, sums) of smp DiceLoss(mode="multiclass"); ``options`` None = smp's defaults through the plain entry point.  This and
    the five functions below serve the whole family: an OverlapOptions selects the Jaccard / Tversky loss on the same sums."""
    _need_cuda(logits, target)
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("dice_loss: contiguous f32 NCHW logits expected")
    if target.dtype != torch.int64 or not target.is_contiguous():
        raise ValueError("dice_loss: contiguous int64 target expected")
    B, K, H, W = logits.shape
    nbytes = _lib.load().gdl_dice_loss_workspace(B, K, H * W)
    sums, loss, ws = _dice_buffers(logits, K, nbytes)
    fn, opt, keep = _dice_entry("loss", "fwd", options)
    fn(_p(logits), _p(target), B, K, H * W, eps, *opt, _p(sums), _p(loss), _p(ws), nbytes, _stream())
    return loss, sums


def dice_loss_bwd(logits: Tensor, target: Tensor, sums: Tensor, upstream: Tensor | None,
                  grad_scale: float = 1.0, eps: float = 1e-7, out: Tensor | None = None,
                  accumulate: bool = False, options: DiceOptions | OverlapOptions | None = None) -> Tensor:
    B, K, H, W = logits.shape
    if out is None:
        out = torch.empty_like(logits)
    fn, opt, keep = _dice_entry("loss", "bwd", options)
    fn(_p(logits), _p(target), B, K, H * W, eps, *opt, _p(sums), _p(upstream), grad_scale, _p(out), int(accumulate),
       _stream())
    return out


def dice_lowres_ok(low: Tensor, size: tuple[int, int]) -> bool:
    """Shapes gdl_dice_loss_lowres_* take: an upsample by at most 64 per direction (DOFA's auxiliary head: 16 x 16 -> 512 x 512), at
    most 16 classes."""
    if low.dim() != 4 or low.shape[3] > 16:
        return False
    hi, wi = low.shape[1], low.shape[2]
    return size[0] >= hi and size[1] >= wi and -(-size[0] // hi) <= 64 and -(-size[1] // wi) <= 64


# gdl_soft_ce_lowres_*, gdl_focal_lowres_* and gdl_cross_entropy_lowres_* take the same shapes
soft_ce_lowres_ok = focal_lowres_ok = cross_entropy_lowres_ok = dice_lowres_ok


def dice_loss_lowres_fwd(low: Tensor, target: Tensor, size: tuple[int, int], eps: float = 1e-7,
                         options: DiceOptions | OverlapOptions | None = None):
    """Dice(multiclass) -- or the family member ``options`` selects -- of bilinear(low -> size) vs target [B, H, W] without the
    full-resolution logits: (loss, sums)."""
    _need_cuda(low, target)
    if low.dtype != torch.float32 or not low.is_contiguous() or low.dim() != 4:
        raise ValueError("dice_loss_lowres: contiguous f32 NHWC low-resolution logits [B, h, w, K] expected")
    B, Hi, Wi, K = low.shape
    if target.dtype != torch.int64 or not target.is_contiguous() or tuple(target.shape) != (B, size[0], size[1]):
        raise ValueError(f"dice_loss_lowres: contiguous int64 target [B, {size[0]}, {size[1]}] expected, got {tuple(target.shape)}")
    nbytes = _lib.load().gdl_dice_loss_lowres_workspace(B, K, size[0], size[1])
    sums, loss, ws = _dice_buffers(low, K, nbytes)
    fn, opt, keep = _dice_entry("loss_lowres", "fwd", options)
    fn(_p(low), _p(target), B, K, Hi, Wi, size[0], size[1], eps, *opt, _p(sums), _p(loss), _p(ws), nbytes, _stream())
    return loss, sums


def dice_loss_lowres_bwd(low: Tensor, target: Tensor, size: tuple[int, int], sums: Tensor, upstream: Tensor | None,
                         grad_scale: float = 1.0, eps: float = 1e-7,
                         options: DiceOptions | OverlapOptions | None = None) -> Tensor:
    B, Hi, Wi, K = low.shape
    dlow = torch.empty_like(low)
    ws, nbytes = _bwd_workspace(_lib.load().gdl_dice_loss_lowres_bwd_workspace, (B, K, Hi, Wi, size[0], size[1]), low)
    fn, opt, keep = _dice_entry("loss_lowres", "bwd", options)
    fn(_p(low), _p(target), B, K, Hi, Wi, size[0], size[1], eps, *opt, _p(sums), _p(upstream), grad_scale, _p(dlow), _p(ws),
       nbytes, _stream())
    return dlow


def dice_binary_loss_fwd(logits: Tensor, target: Tensor, eps: float = 1e-7, options: DiceOptions | OverlapOptions | None = None):
    """smp DiceLoss(mode="binary") -- or the family member ``options`` selects: logits [B,1,H,W] (or any shape) f32, target of
    the same numel, int64 0/1."""
    _need_cuda(logits, target)
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("dice_binary_loss: contiguous f32 logits expected")
    if target.dtype != torch.int64 or not target.is_contiguous() or target.numel() != logits.numel():
        raise ValueError("dice_binary_loss: contiguous int64 target with one entry per logit expected")
    total = logits.numel()
    nbytes = _lib.load().gdl_dice_loss_workspace(1, 1, total)
    sums, loss, ws = _dice_buffers(logits, 1, nbytes)
    fn, opt, keep = _dice_entry("binary_loss", "fwd", options)
    fn(_p(logits), _p(target), total, eps, *opt, _p(sums), _p(loss), _p(ws), nbytes, _stream())
    return loss, sums


def dice_binary_loss_bwd(logits: Tensor, target: Tensor, sums: Tensor, upstream: Tensor | None,
                         grad_scale: float = 1.0, eps: float = 1e-7,
                         options: DiceOptions | OverlapOptions | None = None) -> Tensor:
    out = torch.empty_like(logits)
    fn, opt, keep = _dice_entry("binary_loss", "bwd", options)
    fn(_p(logits), _p(target), logits.numel(), eps, *opt, _p(sums), _p(upstream), grad_scale, _p(out), 0, _stream())
    return out


def dice_binary_lowres_fwd(low: Tensor, target: Tensor, size: tuple[int, int], eps: float = 1e-7,
                           options: DiceOptions | OverlapOptions | None = None):
    """Dice(binary) -- or the family member ``options`` selects -- of bilinear(low -> size) vs target [B, H, W] for the one-class
    head's map [B, h, w, 1], without the full-resolution logits: (loss, sums)."""
    B, Hi, Wi, Ho, Wo = _binary_lowres_check("dice_binary_lowres", low, size, target)
    nbytes = _lib.load().gdl_dice_loss_lowres_workspace(B, 1, Ho, Wo)
    sums, loss, ws = _dice_buffers(low, 1, nbytes)
    fn, opt, keep = _dice_entry("binary_loss_lowres", "fwd", options)
    fn(_p(low), _p(target), B, Hi, Wi, Ho, Wo, eps, *opt, _p(sums), _p(loss), _p(ws), nbytes, _stream())
    return loss, sums


def dice_binary_lowres_bwd(low: Tensor, target: Tensor, size: tuple[int, int], sums: Tensor, upstream: Tensor | None,
                           grad_scale: float = 1.0, eps: float = 1e-7, options: DiceOptions | OverlapOptions | None = None,
                           form: str = "auto") -> Tensor:
    """d loss / d low [B, h, w, 1] * upstream[0] * grad_scale from the forward's ``sums``.  ``form``: "tile" (every full-resolution
    pixel once), "gather" (every shape) or "auto" (the tile kernels where the shape takes them)."""
    B, Hi, Wi, Ho, Wo = _binary_lowres_check("dice_binary_lowres", low, size, target)
    _need_cuda(sums, upstream)
    dlow = torch.empty_like(low)
    lib = _lib.checked()
    ws, nbytes = _bwd_workspace(lib.gdl_binary_lowres_bwd_workspace, (B, Hi, Wi, Ho, Wo), low, form)
    fn, opt, keep = _dice_entry("binary_loss_lowres", "bwd", options)
    fn(_p(low), _p(target), B, Hi, Wi, Ho, Wo, eps, *opt, _p(sums), _p(upstream), grad_scale, _p(dlow), _p(ws), nbytes,
       LOWRES_BWD_FORMS[form], _stream())
    return dlow


class SoftCEOptions(NamedTuple):
    """The constructor options of smp's SoftCrossEntropyLoss as the gdl_soft_ce_* entry points take them: ``smooth_factor`` in
    [0, 1], ``ignore_index`` (any int64, or None) and ``mean`` (reduction "mean": divide by every pixel, ignored ones included)."""

    smooth_factor: float = 0.0
    ignore_index: int | None = -100
    mean: bool = True

    def c_args(self) -> tuple:
        """(smooth, has_ignore, ignore, mean) in the order of the C calls"""
        return (float(self.smooth_factor), int(self.ignore_index is not None), int(self.ignore_index or 0), int(bool(self.mean)))


def soft_ce_fwd(logits: Tensor, target: Tensor, options: SoftCEOptions = SoftCEOptions()) -> Tensor:
    """smp SoftCrossEntropyLoss on NCHW f32 logits [B,K,H,W] and an int64 target [B,H,W]: the loss (0-dim f32)."""
    B, K, HW = _nchw_check("soft_ce", logits, target)
    lib = _lib.checked()
    nbytes = lib.gdl_soft_ce_workspace(B, K, HW)
    loss, _, ws = _loss_buffers(logits, nbytes)
    lib.gdl_soft_ce_fwd(_p(logits), _p(target), B, K, HW, *options.c_args(), _p(loss), _p(ws), nbytes, _stream())
    return loss


def soft_ce_bwd(logits: Tensor, target: Tensor, upstream: Tensor | None, grad_scale: float = 1.0,
                options: SoftCEOptions = SoftCEOptions(), out: Tensor | None = None, accumulate: bool = False) -> Tensor:
    """d loss / d logits * upstream[0] * grad_scale (softmax recomputed from ``logits``); ``out``/``accumulate`` as dice_loss_bwd."""
    B, K, HW = _nchw_check("soft_ce", logits, target)
    _need_cuda(upstream, out)
    out = _grad_out("soft_ce_bwd", logits, out)
    _lib.checked().gdl_soft_ce_bwd(_p(logits), _p(target), B, K, HW, *options.c_args(), _p(upstream), grad_scale, _p(out),
                                   int(accumulate), _stream())
    return out


def soft_ce_lowres_fwd(low: Tensor, target: Tensor, size: tuple[int, int], options: SoftCEOptions = SoftCEOptions(),
                       fused: bool = False):
    """The loss of bilinear(low -> size) vs target [B, H, W] without the full-resolution logits: ``(loss, state)``.  ``fused``: the
    same pass also leaves the unscaled partial patches of d(low) in ``state`` (for soft_ce_lowres_bwd); where the shape does not
    take that form (K > 8, resize close to 1:1), and without ``fused``, ``state`` is None and the backward recomputes."""
    dims = _lowres_check("soft_ce_lowres", low, target, size)
    loss = torch.empty((), device=low.device, dtype=torch.float32)
    lib = _lib.checked()
    nstate = lib.gdl_soft_ce_lowres_fused_state(*dims) if fused else 0
    if nstate:
        state = torch.empty(nstate // 8 + 1, device=low.device, dtype=torch.float64)
        lib.gdl_soft_ce_lowres_fused_fwd(_p(low), _p(target), *dims, *options.c_args(), _p(loss), _p(state), state.numel() * 8,
                                         _stream())
        return loss, state
    nbytes = lib.gdl_soft_ce_lowres_workspace(*dims[:2], *dims[4:])
    ws = torch.empty(nbytes // 8, device=low.device, dtype=torch.float64)
    lib.gdl_soft_ce_lowres_fwd(_p(low), _p(target), *dims, *options.c_args(), _p(loss), _p(ws), nbytes, _stream())
    return loss, None


def soft_ce_lowres_bwd(low: Tensor, target: Tensor, size: tuple[int, int], upstream: Tensor | None, grad_scale: float = 1.0,
                       options: SoftCEOptions = SoftCEOptions(), state: Tensor | None = None) -> Tensor:
    """d loss / d low [B, h, w, K] * upstream[0] * grad_scale: the reduce of the forward's patches (``state`` of a fused forward)
    or the recompute form (tile kernel for K <= 8, gather kernel otherwise)."""
    dims = _lowres_check("soft_ce_lowres", low, target, size)
    _need_cuda(upstream, state)
    dlow = torch.empty_like(low)
    lib = _lib.checked()
    if state is not None:
        lib.gdl_soft_ce_lowres_fused_bwd(_p(state), state.numel() * state.element_size(), *dims, int(bool(options.mean)),
                                         _p(upstream), grad_scale, _p(dlow), _stream())
        return dlow
    ws, nbytes = _bwd_workspace(lib.gdl_soft_ce_lowres_bwd_workspace, dims, low)
    lib.gdl_soft_ce_lowres_bwd(_p(low), _p(target), *dims, *options.c_args(), _p(upstream), grad_scale, _p(dlow), _p(ws), nbytes,
                               _stream())
    return dlow


class FocalOptions(NamedTuple):
    """The constructor options of smp's FocalLoss as the gdl_focal_* entry points take them: ``gamma`` >= 0, ``alpha`` in [0, 1]
    or None, ``ignore_index`` (any int64, or None), ``mean`` (reduction "mean": divide by the number of valid pixels) and
    ``reduced_threshold`` in (0, 1] or None."""

    gamma: float = 2.0
    alpha: float | None = None
    ignore_index: int | None = None
    mean: bool = True
    reduced_threshold: float | None = None

    def c_args(self) -> tuple:
        """(gamma, has_alpha, alpha, has_threshold, threshold, has_ignore, ignore, mean) in the order of the C calls"""
        return (float(self.gamma), int(self.alpha is not None), float(self.alpha or 0.0), int(self.reduced_threshold is not None),
                float(self.reduced_threshold or 0.0), int(self.ignore_index is not None), int(self.ignore_index or 0),
                int(bool(self.mean)))


def focal_fwd(logits: Tensor, target: Tensor, options: FocalOptions = FocalOptions()):
    """smp FocalLoss(mode="multiclass") on NCHW f32 logits [B,K,H,W] and an int64 target [B,H,W]: ``(loss, norm)``, the 0-dim f32
    loss and the divisor the kernels formed on the device (1 / valid pixels, or 1 for "sum"), which focal_bwd reads."""
    B, K, HW = _nchw_check("focal", logits, target)
    lib = _lib.checked()
    nbytes = lib.gdl_focal_workspace(B, K, HW)
    loss, norm, ws = _loss_buffers(logits, nbytes, norm=True)
    lib.gdl_focal_fwd(_p(logits), _p(target), B, K, HW, *options.c_args(), _p(loss), _p(norm), _p(ws), nbytes, _stream())
    return loss, norm


def focal_bwd(logits: Tensor, target: Tensor, norm: Tensor, upstream: Tensor | None, grad_scale: float = 1.0,
              options: FocalOptions = FocalOptions(), out: Tensor | None = None, accumulate: bool = False) -> Tensor:
    """d loss / d logits * upstream[0] * grad_scale (recomputed from ``logits``; ``norm`` from focal_fwd); ``out``/``accumulate``
    as soft_ce_bwd."""
    B, K, HW = _nchw_check("focal", logits, target)
    _need_cuda(norm, upstream, out)
    out = _grad_out("focal_bwd", logits, out)
    _lib.checked().gdl_focal_bwd(_p(logits), _p(target), B, K, HW, *options.c_args(), _p(norm), _p(upstream), grad_scale,
                                 _p(out), int(accumulate), _stream())
    return out


def _focal_binary_check(logits: Tensor, target: Tensor) -> None:
    _need_cuda(logits, target)
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("focal_binary: contiguous f32 logits expected")
    if target.dtype != torch.int64 or not target.is_contiguous() or target.numel() != logits.numel() or logits.numel() == 0:
        raise ValueError("focal_binary: contiguous int64 target with one entry per logit expected")


def focal_binary_fwd(logits: Tensor, target: Tensor, options: FocalOptions = FocalOptions()):
    """smp FocalLoss(mode="binary"): f32 logits of any shape, int64 target of the same numel (1 = positive; any other value that
    is not ``ignore_index`` = negative): ``(loss, norm)`` as focal_fwd."""
    _focal_binary_check(logits, target)
    lib = _lib.checked()
    nbytes = lib.gdl_focal_workspace(1, 1, logits.numel())
    loss, norm, ws = _loss_buffers(logits, nbytes, norm=True)
    lib.gdl_focal_binary_fwd(_p(logits), _p(target), logits.numel(), *options.c_args(), _p(loss), _p(norm), _p(ws), nbytes,
                             _stream())
    return loss, norm


def focal_binary_bwd(logits: Tensor, target: Tensor, norm: Tensor, upstream: Tensor | None, grad_scale: float = 1.0,
                     options: FocalOptions = FocalOptions(), out: Tensor | None = None, accumulate: bool = False) -> Tensor:
    _focal_binary_check(logits, target)
    _need_cuda(norm, upstream, out)
    out = _grad_out("focal_binary_bwd", logits, out)
    _lib.checked().gdl_focal_binary_bwd(_p(logits), _p(target), logits.numel(), *options.c_args(), _p(norm), _p(upstream),
                                        grad_scale, _p(out), int(accumulate), _stream())
    return out


def focal_lowres_fwd(low: Tensor, target: Tensor, size: tuple[int, int], options: FocalOptions = FocalOptions()):
    """The multiclass focal loss of bilinear(low -> size) vs target [B, H, W] without the full-resolution logits:
    ``(loss, norm)`` as focal_fwd."""
    dims = _lowres_check("focal_lowres", low, target, size)
    lib = _lib.checked()
    nbytes = lib.gdl_focal_lowres_workspace(*dims[:2], *dims[4:])
    loss, norm, ws = _loss_buffers(low, nbytes, norm=True)
    lib.gdl_focal_lowres_fwd(_p(low), _p(target), *dims, *options.c_args(), _p(loss), _p(norm), _p(ws), nbytes, _stream())
    return loss, norm


def focal_lowres_bwd(low: Tensor, target: Tensor, size: tuple[int, int], norm: Tensor, upstream: Tensor | None,
                     grad_scale: float = 1.0, options: FocalOptions = FocalOptions(), form: str = "auto") -> Tensor:
    """d loss / d low [B, h, w, K] * upstream[0] * grad_scale.  ``form``: "tile" (K <= 8: every full-resolution element once),
    "gather" (every K <= 16) or "auto" (the tile kernel where the shape takes it, the default -- DESIGN.md section 2)."""
    dims = _lowres_check("focal_lowres", low, target, size)
    _need_cuda(norm, upstream)
    dlow = torch.empty_like(low)
    lib = _lib.checked()
    ws, nbytes = _bwd_workspace(lib.gdl_focal_lowres_bwd_workspace, dims, low, form)
    lib.gdl_focal_lowres_bwd(_p(low), _p(target), *dims, *options.c_args(), _p(norm), _p(upstream), grad_scale, _p(dlow), _p(ws),
                             nbytes, LOWRES_BWD_FORMS[form], _stream())
    return dlow


def focal_binary_lowres_fwd(low: Tensor, target: Tensor, size: tuple[int, int], options: FocalOptions = FocalOptions()):
    """The binary focal loss (z = [y == 1]) of bilinear(low -> size) vs target [B, H, W] for the one-class head's map [B, h, w, 1],
    without the full-resolution logits: ``(loss, norm)`` as focal_fwd."""
    B, Hi, Wi, Ho, Wo = _binary_lowres_check("focal_binary_lowres", low, size, target)
    lib = _lib.checked()
    nbytes = lib.gdl_focal_lowres_workspace(B, 1, Ho, Wo)
    loss, norm, ws = _loss_buffers(low, nbytes, norm=True)
    lib.gdl_focal_binary_lowres_fwd(_p(low), _p(target), B, Hi, Wi, Ho, Wo, *options.c_args(), _p(loss), _p(norm), _p(ws), nbytes,
                                    _stream())
    return loss, norm


def focal_binary_lowres_bwd(low: Tensor, target: Tensor, size: tuple[int, int], norm: Tensor, upstream: Tensor | None,
                            grad_scale: float = 1.0, options: FocalOptions = FocalOptions(), form: str = "auto") -> Tensor:
    """d loss / d low [B, h, w, 1] * upstream[0] * grad_scale; ``form`` as dice_binary_lowres_bwd."""
    B, Hi, Wi, Ho, Wo = _binary_lowres_check("focal_binary_lowres", low, size, target)
    _need_cuda(norm, upstream)
    dlow = torch.empty_like(low)
    lib = _lib.checked()
    ws, nbytes = _bwd_workspace(lib.gdl_binary_lowres_bwd_workspace, (B, Hi, Wi, Ho, Wo), low, form)
    lib.gdl_focal_binary_lowres_bwd(_p(low), _p(target), B, Hi, Wi, Ho, Wo, *options.c_args(), _p(norm), _p(upstream), grad_scale,
                                    _p(dlow), _p(ws), nbytes, LOWRES_BWD_FORMS[form], _stream())
    return dlow


class CrossEntropyOptions(NamedTuple):
    """The constructor options of torch's CrossEntropyLoss as the gdl_cross_entropy_* entry points take them: ``label_smoothing`` in
    [0, 1], ``ignore_index`` (any int64, or None), ``mean`` (reduction "mean": divide by the summed weights of the valid pixels'
    classes) and the device tensor ``weight`` (f32, one value per class, or None), which the kernels read through its pointer at
    call time."""

    label_smoothing: float = 0.0
    ignore_index: int | None = -100
    mean: bool = True
    weight: Tensor | None = None

    def c_args(self) -> tuple:
        """(weight, smooth, has_ignore, ignore, mean) in the order of the C calls"""
        return (_p(self.weight), float(self.label_smoothing), int(self.ignore_index is not None), int(self.ignore_index or 0),
                int(bool(self.mean)))


def _cross_entropy_weight_check(who: str, options: CrossEntropyOptions, K: int) -> None:
    w = options.weight
    if w is not None:
        _need_cuda(w)
        if w.dtype != torch.float32 or not w.is_contiguous() or w.dim() != 1 or w.numel() != K:
            raise ValueError(f"{who}: weight must be a contiguous 1-D f32 tensor of {K} (classes) values, got {tuple(w.shape)} {w.dtype}")


def cross_entropy_fwd(logits: Tensor, target: Tensor, options: CrossEntropyOptions = CrossEntropyOptions()):
    """torch CrossEntropyLoss on NCHW f32 logits [B,K,H,W] and an int64 target [B,H,W]: ``(loss, norm)``, the 0-dim f32 loss and
    the divisor the kernels formed on the device (1 / summed weights of the valid pixels, 0 where that sum is 0, or 1 for "sum"),
    which cross_entropy_bwd reads."""
    B, K, HW = _nchw_check("cross_entropy", logits, target)
    _cross_entropy_weight_check("cross_entropy", options, K)
    lib = _lib.checked()
    nbytes = lib.gdl_cross_entropy_workspace(B, K, HW)
    loss, norm, ws = _loss_buffers(logits, nbytes, norm=True)
    lib.gdl_cross_entropy_fwd(_p(logits), _p(target), B, K, HW, *options.c_args(), _p(loss), _p(norm), _p(ws), nbytes,
                              _stream())
    return loss, norm


def cross_entropy_bwd(logits: Tensor, target: Tensor, norm: Tensor, upstream: Tensor | None, grad_scale: float = 1.0,
                      options: CrossEntropyOptions = CrossEntropyOptions(), out: Tensor | None = None,
                      accumulate: bool = False) -> Tensor:
    """d loss / d logits * upstream[0] * grad_scale (softmax recomputed from ``logits``; ``norm`` from cross_entropy_fwd);
    ``out``/``accumulate`` as soft_ce_bwd."""
    B, K, HW = _nchw_check("cross_entropy", logits, target)
    _cross_entropy_weight_check("cross_entropy", options, K)
    _need_cuda(norm, upstream, out)
    out = _grad_out("cross_entropy_bwd", logits, out)
    _lib.checked().gdl_cross_entropy_bwd(_p(logits), _p(target), B, K, HW, *options.c_args(), _p(norm), _p(upstream), grad_scale,
                                         _p(out), int(accumulate), _stream())
    return out


def cross_entropy_lowres_fwd(low: Tensor, target: Tensor, size: tuple[int, int],
                             options: CrossEntropyOptions = CrossEntropyOptions()):
    """The cross-entropy of bilinear(low -> size) vs target [B, H, W] without the full-resolution logits: ``(loss, norm)`` as
    cross_entropy_fwd."""
    dims = _lowres_check("cross_entropy_lowres", low, target, size)
    _cross_entropy_weight_check("cross_entropy_lowres", options, dims[1])
    lib = _lib.checked()
    nbytes = lib.gdl_cross_entropy_lowres_workspace(*dims[:2], *dims[4:])
    loss, norm, ws = _loss_buffers(low, nbytes, norm=True)
    lib.gdl_cross_entropy_lowres_fwd(_p(low), _p(target), *dims, *options.c_args(), _p(loss), _p(norm), _p(ws), nbytes,
                                     _stream())
    return loss, norm


def cross_entropy_lowres_bwd(low: Tensor, target: Tensor, size: tuple[int, int], norm: Tensor, upstream: Tensor | None,
                             grad_scale: float = 1.0, options: CrossEntropyOptions = CrossEntropyOptions(),
                             form: str = "auto") -> Tensor:
    """d loss / d low [B, h, w, K] * upstream[0] * grad_scale; ``form`` as focal_lowres_bwd."""
    dims = _lowres_check("cross_entropy_lowres", low, target, size)
    _cross_entropy_weight_check("cross_entropy_lowres", options, dims[1])
    _need_cuda(norm, upstream)
    dlow = torch.empty_like(low)
    lib = _lib.checked()
    ws, nbytes = _bwd_workspace(lib.gdl_cross_entropy_lowres_bwd_workspace, dims, low, form)
    lib.gdl_cross_entropy_lowres_bwd(_p(low), _p(target), *dims, *options.c_args(), _p(norm), _p(upstream), grad_scale, _p(dlow),
                                     _p(ws), nbytes, LOWRES_BWD_FORMS[form], _stream())
    return dlow


class SoftBCEOptions(NamedTuple):
    """The constructor options of smp's SoftBCEWithLogitsLoss as the gdl_soft_bce_* entry points take them: ``smooth_factor`` in
    [0, 1] or None, ``ignore_index`` (any int64, or None), ``mean`` (reduction "mean": divide by EVERY element, ignored ones
    included) and the device tensors ``weight`` / ``pos_weight`` (f32, one value or one per channel, or None), which the kernels read
    through their pointers at call time."""

    smooth_factor: float | None = None
    ignore_index: int | None = -100
    mean: bool = True
    weight: Tensor | None = None
    pos_weight: Tensor | None = None

    def c_args(self, numel: int) -> tuple:
        """(has_smooth, smooth, has_ignore, ignore, ignore_f, weight, weight_numel, pos_weight, pos_weight_numel, scale) in the
        order of the C calls; ``numel``: the number of logits (the divisor of "mean")"""
        ign = int(self.ignore_index or 0)
        return (int(self.smooth_factor is not None), float(self.smooth_factor or 0.0), int(self.ignore_index is not None), ign,
                float(ign), _p(self.weight), 0 if self.weight is None else self.weight.numel(), _p(self.pos_weight),
                0 if self.pos_weight is None else self.pos_weight.numel(), 1.0 / numel if self.mean else 1.0)


# dtype -> the `target_type` tag of gdl_soft_bce_*
BCE_TARGET_TYPES = {torch.int64: _lib.BCE_TARGET_I64, torch.float32: _lib.BCE_TARGET_F32}


def _soft_bce_options_check(who: str, options: SoftBCEOptions, C_: int) -> None:
    for name, t in (("weight", options.weight), ("pos_weight", options.pos_weight)):
        if t is None:
            continue
        _need_cuda(t)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() not in (1, C_):
            raise ValueError(f"{who}: {name} must be a contiguous f32 tensor of 1 or {C_} (channels) values, got {tuple(t.shape)} {t.dtype}")


def _soft_bce_check(who: str, logits: Tensor, target: Tensor, options: SoftBCEOptions) -> tuple:
    """(B, C, HW) of NCHW logits [B, C, H, W]; the target holds one value per logit, int64 or f32."""
    _need_cuda(logits, target)
    if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() != 4 or logits.numel() == 0:
        raise ValueError(f"{who}: contiguous f32 NCHW logits [B, C, H, W] expected, got {tuple(logits.shape)} {logits.dtype}")
    if target.dtype not in BCE_TARGET_TYPES or not target.is_contiguous() or target.numel() != logits.numel():
        raise ValueError(f"{who}: contiguous int64 or f32 target with one value per logit expected, got {tuple(target.shape)} {target.dtype}")
    B, C_, H, W = logits.shape
    _soft_bce_options_check(who, options, C_)
    return B, C_, H * W


def soft_bce_fwd(logits: Tensor, target: Tensor, options: SoftBCEOptions = SoftBCEOptions()) -> Tensor:
    """smp SoftBCEWithLogitsLoss on NCHW f32 logits [B,C,H,W] and an int64 or f32 target of the same numel: the loss (0-dim f32)."""
    B, C_, HW = _soft_bce_check("soft_bce", logits, target, options)
    lib = _lib.checked()
    nbytes = lib.gdl_soft_bce_workspace(B, C_, HW)
    loss, _, ws = _loss_buffers(logits, nbytes)
    lib.gdl_soft_bce_fwd(_p(logits), _p(target), BCE_TARGET_TYPES[target.dtype], B, C_, HW, *options.c_args(logits.numel()),
                         _p(loss), _p(ws), nbytes, _stream())
    return loss


def soft_bce_bwd(logits: Tensor, target: Tensor, upstream: Tensor | None, grad_scale: float = 1.0,
                 options: SoftBCEOptions = SoftBCEOptions(), out: Tensor | None = None, accumulate: bool = False) -> Tensor:
    """d loss / d logits * upstream[0] * grad_scale (recomputed from ``logits``); ``out``/``accumulate`` as soft_ce_bwd."""
    B, C_, HW = _soft_bce_check("soft_bce", logits, target, options)
    _need_cuda(upstream, out)
    out = _grad_out("soft_bce_bwd", logits, out)
    _lib.checked().gdl_soft_bce_bwd(_p(logits), _p(target), BCE_TARGET_TYPES[target.dtype], B, C_, HW,
                                    *options.c_args(logits.numel()), _p(upstream), grad_scale, _p(out), int(accumulate), _stream())
    return out


def _soft_bce_lowres_check(low: Tensor, target: Tensor, size: tuple[int, int], options: SoftBCEOptions) -> tuple:
    """(B, Hi, Wi, Ho, Wo) of the one-class map [B, h, w, 1] and a target [B, H, W], int64 or f32."""
    B, Hi, Wi, Ho, Wo = _binary_lowres_check("soft_bce_lowres", low, size)
    _need_cuda(target)
    if target.dtype not in BCE_TARGET_TYPES or not target.is_contiguous() or tuple(target.shape) != (B, Ho, Wo):
        raise ValueError(f"soft_bce_lowres: contiguous int64 or f32 target {[B, Ho, Wo]} expected, got {tuple(target.shape)} {target.dtype}")
    _soft_bce_options_check("soft_bce_lowres", options, 1)
    return B, Hi, Wi, Ho, Wo


def soft_bce_lowres_fwd(low: Tensor, target: Tensor, size: tuple[int, int], options: SoftBCEOptions = SoftBCEOptions()) -> Tensor:
    """The loss of bilinear(low -> size) vs target [B, H, W] for the one-class head's map [B, h, w, 1], without the full-resolution
    logits: the loss (0-dim f32)."""
    B, Hi, Wi, Ho, Wo = _soft_bce_lowres_check(low, target, size, options)
    lib = _lib.checked()
    nbytes = lib.gdl_soft_bce_lowres_workspace(B, Ho, Wo)
    loss, _, ws = _loss_buffers(low, nbytes)
    lib.gdl_soft_bce_lowres_fwd(_p(low), _p(target), BCE_TARGET_TYPES[target.dtype], B, Hi, Wi, Ho, Wo,
                                *options.c_args(target.numel()), _p(loss), _p(ws), nbytes, _stream())
    return loss


def soft_bce_lowres_bwd(low: Tensor, target: Tensor, size: tuple[int, int], upstream: Tensor | None, grad_scale: float = 1.0,
                        options: SoftBCEOptions = SoftBCEOptions(), form: str = "auto") -> Tensor:
    """d loss / d low [B, h, w, 1] * upstream[0] * grad_scale; ``form`` as dice_binary_lowres_bwd."""
    B, Hi, Wi, Ho, Wo = _soft_bce_lowres_check(low, target, size, options)
    _need_cuda(upstream)
    dlow = torch.empty_like(low)
    lib = _lib.checked()
    ws, nbytes = _bwd_workspace(lib.gdl_binary_lowres_bwd_workspace, (B, Hi, Wi, Ho, Wo), low, form)
    lib.gdl_soft_bce_lowres_bwd(_p(low), _p(target), BCE_TARGET_TYPES[target.dtype], B, Hi, Wi, Ho, Wo,
                                *options.c_args(target.numel()), _p(upstream), grad_scale, _p(dlow), _p(ws), nbytes,
                                LOWRES_BWD_FORMS[form], _stream())
    return dlow


class LovaszOptions(NamedTuple):
    """The constructor options of smp's LovaszLoss as the gdl_lovasz_* entry points take them: ``per_image`` (one sort per image
    and class, the loss averaged over images) and ``ignore_index`` (any int64, or None)."""

    per_image: bool = False
    ignore_index: int | None = None

    def c_args(self) -> tuple:
        """(per_image, has_ignore, ignore) in the order of the C calls"""
        return (int(bool(self.per_image)), int(self.ignore_index is not None), int(self.ignore_index or 0))


def sort_desc_f32(keys: Tensor):
    """Stable descending sort of non-negative f32 keys [S, n] along dim 1 by the library's segmented radix sort: ``(sorted, perm)``
    with ``perm`` int32, bit for bit ``torch.sort(keys, dim=1, descending=True, stable=True)`` (NaN and negative keys unspecified)."""
    _need_cuda(keys)
    if keys.dtype != torch.float32 or not keys.is_contiguous() or keys.dim() != 2:
        raise ValueError("sort_desc_f32: contiguous f32 keys [S, n] expected")
    S, n = keys.shape
    out, perm = torch.empty_like(keys), torch.empty(S, n, device=keys.device, dtype=torch.int32)
    lib = _lib.checked()
    nbytes = lib.gdl_sort_desc_workspace(S, n)
    ws = torch.empty(nbytes // 8, device=keys.device, dtype=torch.float64)
    lib.gdl_sort_desc_f32(_p(keys), S, n, _p(out), _p(perm), _p(ws), nbytes, _stream())
    return out, perm


def _lovasz_out(like: Tensor, lib, segs: int, n: int, K: int):
    """(loss [], coef like the logits, norm [segs], workspace, its bytes) for a Lovasz forward, on ``like``'s device."""
    nbytes = lib.gdl_lovasz_workspace(segs, n, K)
    return (torch.empty((), device=like.device, dtype=torch.float32), torch.empty(like.numel(), device=like.device, dtype=torch.float32),
            torch.empty(max(segs, 1), device=like.device, dtype=torch.float32),
            torch.empty(nbytes // 8, device=like.device, dtype=torch.float64), nbytes)


def lovasz_fwd(logits: Tensor, target: Tensor, options: LovaszOptions = LovaszOptions()):
    """smp LovaszLoss(mode="multiclass") on NCHW f32 logits [B,K,H,W] and an int64 target [B,H,W]: ``(loss, coef, norm)``, the 0-dim
    f32 loss, the Jaccard coefficient of every (class, pixel) in pixel order and the weight of every segment in the loss (formed on
    the device), both of which lovasz_bwd reads."""
    B, K, HW = _nchw_check("lovasz", logits, target)
    lib = _lib.checked()
    segs, n = (B * K, HW) if options.per_image else (K, B * HW)
    loss, coef, norm, ws, nbytes = _lovasz_out(logits, lib, segs, n, K)
    lib.gdl_lovasz_fwd(_p(logits), _p(target), B, K, HW, *options.c_args(), _p(loss), _p(coef), _p(norm), _p(ws), nbytes,
                       _stream())
    return loss, coef, norm


def lovasz_bwd(logits: Tensor, target: Tensor, coef: Tensor, norm: Tensor, upstream: Tensor | None, grad_scale: float = 1.0,
               options: LovaszOptions = LovaszOptions(), out: Tensor | None = None, accumulate: bool = False) -> Tensor:
    """d loss / d logits * upstream[0] * grad_scale (softmax recomputed from ``logits``; ``coef``, ``norm`` from lovasz_fwd with the
    same options); ``out``/``accumulate`` as focal_bwd."""
    B, K, HW = _nchw_check("lovasz", logits, target)
    _need_cuda(coef, norm, upstream, out)
    _f32vec(coef, logits.numel(), "lovasz_bwd: coef")
    _f32vec(norm, B * K if options.per_image else K, "lovasz_bwd: norm")
    out = _grad_out("lovasz_bwd", logits, out)
    _lib.checked().gdl_lovasz_bwd(_p(logits), _p(target), B, K, HW, *options.c_args(), _p(coef), _p(norm), _p(upstream), grad_scale,
                                  _p(out), int(accumulate), _stream())
    return out


def _lovasz_binary_check(logits: Tensor, target: Tensor) -> tuple[int, int]:
    _need_cuda(logits, target)
    if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() < 1:
        raise ValueError("lovasz_binary: contiguous f32 logits [B, ...] expected")
    if target.dtype != torch.int64 or not target.is_contiguous() or target.numel() != logits.numel() or logits.numel() == 0:
        raise ValueError("lovasz_binary: contiguous int64 target with one entry per logit expected")
    return logits.shape[0], logits.numel() // logits.shape[0]


def lovasz_binary_fwd(logits: Tensor, target: Tensor, options: LovaszOptions = LovaszOptions()):
    """smp LovaszLoss(mode="binary"): f32 logits [B, ...], int64 target of the same numel (1 = positive; any other value that is not
    ``ignore_index`` = negative): ``(loss, coef, norm)`` as lovasz_fwd."""
    B, per = _lovasz_binary_check(logits, target)
    lib = _lib.checked()
    segs, n = (B, per) if options.per_image else (1, B * per)
    loss, coef, norm, ws, nbytes = _lovasz_out(logits, lib, segs, n, 1)
    lib.gdl_lovasz_binary_fwd(_p(logits), _p(target), B, per, *options.c_args(), _p(loss), _p(coef), _p(norm), _p(ws), nbytes,
                              _stream())
    return loss, coef, norm


def lovasz_binary_bwd(logits: Tensor, target: Tensor, coef: Tensor, norm: Tensor, upstream: Tensor | None, grad_scale: float = 1.0,
                      options: LovaszOptions = LovaszOptions(), out: Tensor | None = None, accumulate: bool = False) -> Tensor:
    B, per = _lovasz_binary_check(logits, target)
    _need_cuda(coef, norm, upstream, out)
    _f32vec(coef, logits.numel(), "lovasz_binary_bwd: coef")
    _f32vec(norm, B if options.per_image else 1, "lovasz_binary_bwd: norm")
    out = _grad_out("lovasz_binary_bwd", logits, out)
    _lib.checked().gdl_lovasz_binary_bwd(_p(logits), _p(target), B, per, *options.c_args(), _p(coef), _p(norm), _p(upstream),
                                         grad_scale, _p(out), int(accumulate), _stream())
    return out


# ------------------------------------------------------------------ optimizer
def sumsq_accum(x: Tensor, acc: Tensor) -> None:
    _lib.checked().gdl_sumsq(_p(x), x.numel(), _p(acc), _stream())


def clip_coef(sumsq: Tensor, max_norm: float, coef: Tensor) -> None:
    _lib.checked().gdl_clip_coef(_p(sumsq), max_norm, _p(coef), _stream())


def multi_sumsq(table: Tensor, acc: Tensor) -> None:
    """acc += sum of squares of every gradient chunk listed in the device table [nchunks, 5]."""
    _lib.checked().gdl_multi_sumsq(_p(table), table.shape[0], _p(acc), _stream())


def multi_adam(table: Tensor, lr: float, b1: float, b2: float, eps: float, wd: float, step: int,
               clip: Tensor | None) -> None:
    bc1, bc2 = 1.0 - b1**step, 1.0 - b2**step
    _lib.checked().gdl_multi_adam(_p(table), table.shape[0], lr, b1, b2, eps, wd, bc1, bc2, _p(clip),
                                  _stream())


def adam_tick(state: Tensor, b1: float, b2: float) -> None:
    """state[0] += 1 and the two bias corrections refreshed, on the device (capturable Adam, see gdl_adam_tick)."""
    _lib.checked().gdl_adam_tick(_p(state), float(b1), float(b2), _stream())


def multi_adam_dev(table: Tensor, state: Tensor, clip: Tensor | None) -> None:
    _lib.checked().gdl_multi_adam_dev(_p(table), table.shape[0], _p(state), _p(clip), _stream())


def multi_adamw(table: Tensor, lr: float, b1: float, b2: float, eps: float, wd: float, step: int,
                clip: Tensor | None) -> None:
    """torch.optim.AdamW (decoupled weight decay) over the chunk table, see gdl_multi_adamw."""
    bc1, bc2 = 1.0 - b1**step, 1.0 - b2**step
    _lib.checked().gdl_multi_adamw(_p(table), table.shape[0], lr, b1, b2, eps, wd, bc1, bc2, _p(clip),
                                   _stream())


def multi_adamw_dev(table: Tensor, state: Tensor, clip: Tensor | None) -> None:
    _lib.checked().gdl_multi_adamw_dev(_p(table), table.shape[0], _p(state), _p(clip), _stream())


def multi_sgd(table: Tensor, lr: float, momentum: float, dampening: float, nesterov: bool, wd: float, step: int,
              clip: Tensor | None) -> None:
    """torch.optim.SGD over the chunk table, see gdl_multi_sgd; ``step`` = the step count of the table's parameters (the
    momentum buffer is the gradient itself at step 1)."""
    _lib.checked().gdl_multi_sgd(_p(table), table.shape[0], lr, momentum, dampening, int(bool(nesterov)), wd, int(step == 1),
                                 _p(clip), _stream())


def sgd_tick(state: Tensor) -> None:
    """state[0] += 1 and the first-step flag refreshed, on the device (capturable SGD, see gdl_sgd_tick)."""
    _lib.checked().gdl_sgd_tick(_p(state), _stream())


def multi_sgd_dev(table: Tensor, state: Tensor, clip: Tensor | None) -> None:
    _lib.checked().gdl_multi_sgd_dev(_p(table), table.shape[0], _p(state), _p(clip), _stream())


def multi_repack(table: Tensor, total_tiles: int) -> None:
    """Rebuild the bf16 operands derived from 3x3 conv parameters (channel-slice, tap-major, data-gradient layouts) listed in
    ``table`` (device int64 [rows, 10], see gdl_multi_repack) in one launch."""
    _lib.checked().gdl_multi_repack(_p(table), table.shape[0], int(total_tiles), _stream())


def adam_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, lr: float, b1: float, b2: float,
              eps: float, wd: float, step: int, clip: Tensor | None) -> None:
    bc1, bc2 = 1.0 - b1**step, 1.0 - b2**step
    _lib.checked().gdl_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, b1, b2, eps, wd, bc1,
                                 bc2, _p(clip), _stream())


# raster preparation (include/gdlhip_raster.h): a raster put on another grid, and the sums of the dataset statistics
RASTER_METHODS = {"nearest": _lib.RASTER_NEAREST, "bilinear": _lib.RASTER_BILINEAR, "cubic": _lib.RASTER_CUBIC}
RASTER_STATS_DRAIN_PIXELS = 1 << 30      # RasterStats drains its device accumulator before this many pixels per band are in it


def _raster_check(op: str, src) -> tuple[int, int, int]:
    if not isinstance(src, Tensor) or src.dtype not in _RAW_KIND or src.dim() != 3 or not src.is_contiguous() or src.numel() < 1:
        got = f"{src.dtype} {tuple(src.shape)}" if isinstance(src, Tensor) else type(src).__name__
        raise ValueError(f"{op}: contiguous non-empty [C, H, W] uint8/uint16/int16/float32 raster expected, got {got}")
    Cc, H, W = (int(n) for n in src.shape)
    if H * W >= 1 << 31 or Cc > 65535:
        raise ValueError(f"{op}: raster {tuple(src.shape)}: H * W must stay below 2^31 and C below 65536")
    return Cc, H, W


def raster_nodata(op: str, nodata, dtype: torch.dtype, channels: int):
    """(values, present) as the HOST arrays gdl_raster_warp / gdl_raster_stats read, or (None, None) without nodata: ``nodata`` is
    None, one number, or one entry per band of which any may be None (that band has no nodata).  The numbers are held against
    ``dtype`` by ``scene_nodata_values`` (a value no sample can hold is a ValueError; a float32 raster compares after rounding
    to float32, and takes NaN: then a NaN sample is nodata)."""
    if nodata is None:
        return None, None
    if isinstance(nodata, Tensor):
        nodata = nodata.detach().cpu().tolist()
    entries = list(nodata) if isinstance(nodata, (list, tuple)) else [nodata] * channels
    if len(entries) != channels:
        raise ValueError(f"{op}: {len(entries)} nodata values for {channels} bands")
    present = [e is not None for e in entries]
    if not any(present):
        return None, None
    given = scene_nodata_values([e for e in entries if e is not None], dtype, sum(present), op).tolist()
    values = iter(given)
    return ((C.c_double * channels)(*[next(values) if p else 0.0 for p in present]), (C.c_uint8 * channels)(*[int(p) for p in present]))


def _dst_nodata_check(op: str, dst_nodata, dtype: torch.dtype) -> float:
    if isinstance(dst_nodata, bool) or not isinstance(dst_nodata, (int, float)):
        raise ValueError(f"{op}: dst_nodata must be a number, got {dst_nodata!r}")
    if dtype in _RAW_LIMITS:
        lo, hi = _RAW_LIMITS[dtype]
        if dst_nodata != dst_nodata or abs(dst_nodata) == float("inf") or dst_nodata != int(dst_nodata) or not lo <= dst_nodata <= hi:
            raise ValueError(f"{op}: dst_nodata {dst_nodata!r} is not a value of {dtype}")
    return float(dst_nodata)


def raster_warp(src: Tensor, dst_shape: tuple[int, int], sx: float, ox: float, sy: float, oy: float, method: str = "bilinear",
                nodata=None, dst_nodata: float = 0, out_dtype: torch.dtype | None = None, return_valid: bool = False):
    """``src`` [C, H, W] (uint8/uint16/int16/float32, on the device) resampled onto a grid of ``dst_shape`` = (Hd, Wd) whose pixel
    (y, x) lies at the source pixel coordinates u = (x + 0.5) sx + ox, v = (y + 0.5) sy + oy (sx, sy > 0): [C, Hd, Wd] of
    ``out_dtype`` (the source's, the default, or float32), and with ``return_valid`` also the uint8 [C, Hd, Wd] validity planes
    (gdl_raster_warp; the rule is stated in include/gdlhip_raster.h).  ``method``: "nearest", "bilinear" or "cubic"; the last
    two widen with the scale (an antialiased resize) up to a scale of 16.  ``nodata``: None, one number or one per band (None for
    a band without); a masked sample takes no part, and a pixel whose centre falls on a masked sample or outside the source, or
    whose unmasked taps carry less than a quarter of the weight, takes ``dst_nodata``.

    A NaN nodata means "a NaN sample", as in ``scene_valid``.  This departs from the reference, whose ``band != nan``
    (utils/rasters.py:129) excludes nothing.  The resampling is this library's own and is not GDAL's."""
    op = "raster_warp"
    Cc, H, W = _raster_check(op, src)
    if method not in RASTER_METHODS:
        raise ValueError(f"{op}: unknown method {method!r} ('nearest', 'bilinear' or 'cubic')")
    out_dtype = src.dtype if out_dtype is None else out_dtype
    if out_dtype not in (src.dtype, torch.float32):
        raise ValueError(f"{op}: out_dtype must be the source's ({src.dtype}) or torch.float32, got {out_dtype}")
    try:
        Hd, Wd = (int(n) for n in dst_shape)
    except (TypeError, ValueError):
        raise ValueError(f"{op}: dst_shape must be (Hd, Wd), got {dst_shape!r}") from None
    if Hd < 1 or Wd < 1 or Hd * Wd >= 1 << 31:
        raise ValueError(f"{op}: dst_shape {dst_shape!r}: sizes must be positive and Hd * Wd below 2^31")
    values, present = raster_nodata(op, nodata, src.dtype, Cc)
    fill = _dst_nodata_check(op, dst_nodata, out_dtype)
    geometry = tuple(float(g) for g in (sx, ox, sy, oy))
    lib, kind = _lib.checked(), RASTER_METHODS[method]
    nbytes = lib.gdl_raster_warp_workspace(Hd, Wd, geometry[0], geometry[2], kind)
    if nbytes < 0:
        check(-1, op)
    _need_cuda(src)
    dev = src.device
    ws = torch.empty(((nbytes + 7) // 8,), device=dev, dtype=torch.float64) if nbytes else None      # the tap tables
    dst =torch.empty((Cc, Hd, Wd), device=dev, dtype=out_dtype)
    valid = torch.empty((Cc, Hd, Wd), device=dev, dtype=torch.uint8) if return_valid else None
    lib.gdl_raster_warp(_p(src), _RAW_KIND[src.dtype], Cc, H, W, Hd, Wd, *geometry, kind, values, present, fill, _p(dst),
                        _RAW_KIND[out_dtype], _p(valid), _p(ws), _stream())
    return (dst, valid) if return_valid else dst


class RasterStats:
    """The per-band count, sum and sum of squares of the valid samples of any number of rasters: a device accumulator that
    ``raster_stats`` adds to (gdl_raster_stats), drained into Python numbers (exact integers for the integer rasters, floats for
    float32) before ``RASTER_STATS_DRAIN_PIXELS`` pixels per band are in it, so that a uint16 sum of squares never wraps its 64
    bits.  ``finish()`` gives (means, stds)."""

    def __init__(self) -> None:
        self.dtype = None            # of the rasters: the first one's
        self.acc = None              # int64 [C, 3] on the device (words 1 and 2 hold float64 for float32 rasters)
        self.pending = 0             # pixels per band added since the last drain
        self.count, self.total, self.total_sq = [], [], []

    @classmethod
    def from_sums(cls, count, total, total_sq) -> "RasterStats":
        """A holder of given sums (one entry per band), no device involved."""
        self = cls()
        self.count, self.total, self.total_sq = list(count), list(total), list(total_sq)
        if not len(self.count) == len(self.total) == len(self.total_sq):
            raise ValueError("RasterStats.from_sums: one count, sum and sum of squares per band")
        return self

    def admit(self, src: Tensor, pixels: int) -> Tensor:
        """The accumulator the next ``pixels`` pixels per band of ``src`` go to, drained first where they would reach the limit."""
        Cc = int(src.shape[0])
        if self.acc is None:
            self.dtype = src.dtype
            self.acc = torch.zeros((Cc, 3), device=src.device, dtype=torch.int64)
            if not self.count:
                self.count, self.total, self.total_sq = [0] * Cc, [0] * Cc, [0] * Cc
        if src.dtype != self.dtype or Cc != len(self.count) or src.device != self.acc.device:
            raise ValueError(f"raster_stats: the accumulator holds {len(self.count)} bands of {self.dtype} on {self.acc.device}, "
                             f"got {Cc} of {src.dtype} on {src.device}")
        if self.pending and self.pending + pixels >= RASTER_STATS_DRAIN_PIXELS:
            self.drain()
        self.pending += pixels
        return self.acc

    def drain(self) -> None:
        """The device accumulator added to the Python sums and zeroed (one device-to-host copy)."""
        if self.acc is None or not self.pending:
            return
        host = self.acc.cpu()
        sums = host.tolist() if self.dtype != torch.float32 else [[int(n), s, q] for (n, _, _), (_, s, q) in
                                                                  zip(host.tolist(), host.view(torch.float64).tolist())]
        for c, (n, s, q) in enumerate(sums):
            self.count[c] += n
            self.total[c] += s
            self.total_sq[c] += q
        self.acc.zero_()
        self.pending = 0

    def finish(self) -> tuple[list[float], list[float]]:
        """(means, stds) per band: mean = sum / N and std = sqrt(sum of squares / N - mean^2), the reference's population formula
        (utils/rasters.py:142-143), from the exact integers where the sums are integers (in rationals, rounded once at the end)
        and in float64 otherwise, a difference below zero (rounding alone) taken as zero.  A band without a valid pixel is a
        ValueError."""
        from fractions import Fraction
        self.drain()
        means, stds = [], []
        for c, (n, s, q) in enumerate(zip(self.count, self.total, self.total_sq)):
            if n <= 0:
                raise ValueError(f"raster statistics: band {c} has no valid pixel")
            if isinstance(s, int) and isinstance(q, int):
                mean = Fraction(s, n)
                var = Fraction(q, n) - mean * mean
                means.append(float(mean))
                stds.append(math.sqrt(var))
            else:
                mean = s / n
                means.append(mean)
                stds.append(math.sqrt(max(q / n - mean * mean, 0.0)))
        return means, stds


def raster_stats(src: Tensor, nodata=None, acc: RasterStats | None = None) -> RasterStats:
    """The count, sum and sum of squares of the samples of ``src`` [C, H, W] (uint8/uint16/int16/float32, on the device) that are
    not their band's ``nodata`` (None, one number or one per band; NaN for float32: the NaN samples), added per band to ``acc``
    (a ``RasterStats``; a new one where None), which is returned (gdl_raster_stats).  Integer rasters are summed exactly in 64-bit
    integers; float32 ones in float64 in a fixed order, the same bits from run to run."""
    op = "raster_stats"
    Cc, H, W = _raster_check(op, src)
    if acc is not None and not isinstance(acc, RasterStats):
        raise ValueError(f"{op}: acc must be a RasterStats, got {type(acc).__name__}")
    values, present = raster_nodata(op, nodata, src.dtype, Cc)
    _need_cuda(src)
    acc = RasterStats() if acc is None else acc
    words = acc.admit(src, H * W)
    lib, kind = _lib.checked(), _RAW_KIND[src.dtype]
    nbytes = lib.gdl_raster_stats_workspace(kind, Cc, H, W)
    ws = torch.empty((nbytes // 8,), device=src.device, dtype=torch.float64) if nbytes else None
    lib.gdl_raster_stats(_p(src), kind, Cc, H, W, values, present, _p(words), _p(ws), _stream())
    return acc


# raster radiometry (include/gdlhip_raster_tone.h): per-band histograms, quantiles off them, the stretch to uint8 / float32
_HIST_LAYOUT = {torch.uint8: (256, 0.0), torch.uint16: (65536, 0.0), torch.int16: (65536, -32768.0)}      # bins, value of bin 0


def _number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float))


def _hist_binning(op: str, dtype: torch.dtype, channels: int, bins, value_range):
    """(bins, per-band (lo, hi) or None): the fixed layout of an integer dtype, or what the caller gives for float32."""
    if dtype in _HIST_LAYOUT:
        if bins is not None or value_range is not None:
            raise ValueError(f"{op}: bins and value_range are for float32 rasters: the bins of {dtype} are its values")
        return _HIST_LAYOUT[dtype][0], None
    if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= _lib.RASTER_TONE_MAX_BINS:
        raise ValueError(f"{op}: a float32 raster needs bins, an int in 1..{_lib.RASTER_TONE_MAX_BINS}, got {bins!r}")
    pairs = value_range.detach().cpu().tolist() if isinstance(value_range, Tensor) else value_range
    if isinstance(pairs, (list, tuple)) and len(pairs) == 2 and all(_number(v) for v in pairs):
        pairs = [pairs] * channels
    ok = isinstance(pairs, (list, tuple)) and len(pairs) == channels and all(
        isinstance(p, (list, tuple)) and len(p) == 2 and all(_number(v) for v in p) for p in pairs)
    if not ok:
        raise ValueError(f"{op}: a float32 raster needs value_range, one (lo, hi) or one per band ({channels}), got {value_range!r}")
    ranges = [(float(lo), float(hi)) for lo, hi in pairs]
    for lo, hi in ranges:
        if not (math.isfinite(lo) and math.isfinite(hi) and math.isfinite(hi - lo) and lo < hi):
            raise ValueError(f"{op}: value_range ({lo}, {hi}) must be finite with lo < hi")
    return bins, ranges


class RasterHist:
    """The per-band histogram of the valid samples of any number of rasters: a device accumulator int64 [C, bins + 2] that
    ``raster_hist`` adds to (gdl_raster_hist).  ``bins`` and ``ranges`` are its binning: 256 / 65536 / 65536 bins of one value
    each for uint8 / uint16 / int16 (``ranges`` None), or ``bins`` equal bins over each band's (lo, hi) for float32.  The
    accumulator is allocated by the first raster added."""

    def __init__(self, dtype: torch.dtype, channels: int, bins: int, ranges=None) -> None:
        self.dtype, self.channels, self.bins, self.ranges = dtype, int(channels), int(bins), ranges
        self.acc = None

    def admit(self, src: Tensor, bins: int, ranges) -> Tensor:
        """The accumulator for ``src`` with that binning (refused where it is not this one's), allocated on first use."""
        if (src.dtype, int(src.shape[0]), bins, ranges) != (self.dtype, self.channels, self.bins, self.ranges):
            raise ValueError(f"raster_hist: the accumulator holds {self.channels} bands of {self.dtype} in {self.bins} bins over "
                             f"{self.ranges}, got {int(src.shape[0])} of {src.dtype} in {bins} over {ranges}")
        _need_cuda(src)
        if self.acc is None:
            self.acc = torch.zeros((self.channels, self.bins + 2), device=src.device, dtype=torch.int64)
        if self.acc.device != src.device:
            raise ValueError(f"raster_hist: the accumulator is on {self.acc.device}, the raster on {src.device}")
        return self.acc

    def _filled(self) -> Tensor:
        if self.acc is None:
            raise ValueError("RasterHist: no raster has been added yet")
        return self.acc

    @property
    def counts(self) -> Tensor:
        """int64 [C, bins] on the device (a view of the accumulator)."""
        return self._filled()[:, :self.bins]

    @property
    def under(self) -> Tensor:
        """int64 [C]: the float32 samples below their band's range (0 for the integer dtypes)."""
        return self._filled()[:, self.bins]

    @property
    def over(self) -> Tensor:
        return self._filled()[:, self.bins + 1]

    @property
    def total(self) -> Tensor:
        """int64 [C] on the device: the samples in the bins (under and over left out)."""
        return self.counts.sum(dim=1)

    def bin_edges(self) -> tuple[list[float], list[float]]:
        """(origin, step) per band: the value of bin b is origin + b * step (the bin's lower edge for float32)."""
        if self.ranges is None:
            return [_HIST_LAYOUT[self.dtype][1]] * self.channels, [1.0] * self.channels
        return [lo for lo, _ in self.ranges], [(hi - lo) / self.bins for lo, hi in self.ranges]

    def quantiles(self, qs) -> Tensor:
        """float64 [C, Q] on the device: per band the ``qs``-quantiles (each in [0, 1], at most 64) of the valid samples, numpy's
        ``method="lower"`` read off the histogram (gdl_raster_hist_quantiles; exact for the integer dtypes, the lower edge of the
        sample's bin for float32); NaN for a band without a valid sample.  Nothing is copied to the host."""
        qs = [qs] if _number(qs) else list(qs)
        if not 1 <= len(qs) <= _lib.RASTER_TONE_MAX_Q or not all(_number(q) and 0.0 <= q <= 1.0 for q in qs):
            raise ValueError(f"RasterHist.quantiles: 1..{_lib.RASTER_TONE_MAX_Q} numbers in [0, 1] expected, got {qs!r}")
        acc = self._filled()
        origin, step = self.bin_edges()
        out = torch.empty((self.channels, len(qs)), device=acc.device, dtype=torch.float64)
        doubles = C.c_double * self.channels
        _lib.checked().gdl_raster_hist_quantiles(_p(acc), self.channels, self.bins, (C.c_double * len(qs))(*qs), len(qs),
                                                 doubles(*origin), doubles(*step), _p(out), _stream())
        return out

    def percentile_bounds(self, lo_pct: float = 2.0, hi_pct: float = 98.0) -> Tensor:
        """float64 [C, 2] on the device, contiguous: the two percentiles of every band, what ``raster_stretch`` takes as bounds."""
        if not (_number(lo_pct) and _number(hi_pct) and 0.0 <= lo_pct <= hi_pct <= 100.0):
            raise ValueError(f"RasterHist.percentile_bounds: 0 <= lo_pct <= hi_pct <= 100 expected, got {lo_pct!r}, {hi_pct!r}")
        return self.quantiles([lo_pct / 100.0, hi_pct / 100.0])


def raster_hist(src: Tensor, nodata=None, acc: RasterHist | None = None, *, bins: int | None = None, value_range=None) -> RasterHist:
    """The histogram of the samples of ``src`` [C, H, W] (uint8/uint16/int16/float32, on the device) that are not their band's
    ``nodata`` (None, one number or one per band; NaN for float32: the NaN samples), added per band to ``acc`` (a ``RasterHist``
    of the same dtype, band count and binning; a new one where None), which is returned (gdl_raster_hist).  The integer dtypes
    have one bin per value; float32 needs ``bins`` (1..65536) and ``value_range``, one (lo, hi) or one per band: samples below
    and above are counted in ``.under`` / ``.over``, a NaN that is not nodata nowhere.  Exact integer counts, the same bits from
    run to run.  The rule is stated in include/gdlhip_raster_tone.h; the reference has no counterpart."""
    op = "raster_hist"
    Cc, H, W = _raster_check(op, src)
    if acc is not None and not isinstance(acc, RasterHist):
        raise ValueError(f"{op}: acc must be a RasterHist, got {type(acc).__name__}")
    nbins, ranges = _hist_binning(op, src.dtype, Cc, bins, value_range)
    values, present = raster_nodata(op, nodata, src.dtype, Cc)
    acc = RasterHist(src.dtype, Cc, nbins, ranges) if acc is None else acc
    words = acc.admit(src, nbins, ranges)
    doubles = C.c_double * Cc
    lo, hi = (None, None) if ranges is None else (doubles(*[r[0] for r in ranges]), doubles(*[r[1] for r in ranges]))
    _lib.checked().gdl_raster_hist(_p(src), _RAW_KIND[src.dtype], Cc, H, W, values, present, nbins, lo, hi, _p(words), _stream())
    return acc


def raster_stretch(src: Tensor, bounds, out_range=(0, 255), nodata=None, dst_nodata: float = 0,
                   out_dtype: torch.dtype = torch.uint8, return_valid: bool = False):
    """``src`` [C, H, W] (uint8/uint16/int16/float32, on the device) stretched band by band: the band's ``bounds`` (lo, hi) go to
    ``out_range`` = (out_lo, out_hi), linearly in float64 and clipped, as uint8 (rounded half up) or float32 [C, H, W]
    (gdl_raster_stretch; the rule is stated in include/gdlhip_raster_tone.h).  ``bounds``: a float64 [C, 2] tensor on the device
    (``RasterHist.percentile_bounds``: nothing goes through the host) or a host sequence of C (lo, hi) pairs, which is uploaded.
    Where hi <= lo the samples above lo take out_hi and the others out_lo.  A nodata sample (``nodata`` as in ``raster_stats``),
    a NaN sample and every sample of a band whose bounds are NaN take ``dst_nodata``; with ``return_valid`` the uint8 [C, H, W]
    plane that is 0 there comes back too.  There is no gamma."""
    op = "raster_stretch"
    Cc, H, W = _raster_check(op, src)
    if out_dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{op}: out_dtype must be torch.uint8 or torch.float32, got {out_dtype}")
    if not (isinstance(out_range, (list, tuple)) and len(out_range) == 2 and all(_number(v) and math.isfinite(v) for v in out_range)):
        raise ValueError(f"{op}: out_range must be two finite numbers (out_lo, out_hi), got {out_range!r}")
    if out_dtype == torch.uint8 and not all(0 <= v <= 255 for v in out_range):
        raise ValueError(f"{op}: out_range {tuple(out_range)!r} must lie in 0..255 for a uint8 destination")
    fill = _dst_nodata_check(op, dst_nodata, out_dtype)
    values, present = raster_nodata(op, nodata, src.dtype, Cc)
    if isinstance(bounds, Tensor):
        if bounds.dtype != torch.float64 or tuple(bounds.shape) != (Cc, 2) or not bounds.is_contiguous():
            raise ValueError(f"{op}: bounds must be a contiguous float64 [C, 2] = [{Cc}, 2] tensor, got {bounds.dtype} {tuple(bounds.shape)}")
    else:
        pairs = list(bounds) if isinstance(bounds, (list, tuple)) else None
        if pairs is None or len(pairs) != Cc or not all(isinstance(p, (list, tuple)) and len(p) == 2 and all(_number(v) for v in p)
                                                          for p in pairs):
            raise ValueError(f"{op}: bounds must be a float64 [C, 2] tensor or {Cc} (lo, hi) pairs, got {bounds!r}")
        bounds = torch.tensor([[float(lo), float(hi)] for lo, hi in pairs], dtype=torch.float64)
    _need_cuda(src)
    bounds = bounds.to(src.device)
    dst = torch.empty((Cc, H, W), device=src.device, dtype=out_dtype)
    valid = torch.empty((Cc, H, W), device=src.device, dtype=torch.uint8) if return_valid else None
    _lib.checked().gdl_raster_stretch(_p(src), _RAW_KIND[src.dtype], Cc, H, W, values, present, _p(bounds), float(out_range[0]),
                                      float(out_range[1]), fill, _p(dst), _RAW_KIND[out_dtype], _p(valid), _stream())
    return (dst, valid) if return_valid else dst
