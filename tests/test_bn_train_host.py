"""The train-mode BatchNorm protocol around a convolution (gdlhip.nn / gdlhip.cnn autograd nodes), pinned on the CPU:

    forward:  local statistics -> count-weighted cross-rank merge -> running-estimate update -> fold-cache invalidation
    backward: sums pass -> one all-reduce of the pair -> rescale to the global count -> dx pass

Every ``gdlhip.ops`` function these nodes launch is replaced by a stand-in that records its name and computes the same
arithmetic in plain torch (``FakeOps``), so each case pins the ORDER of the launches, the two SYNC_MESSAGES counters and the
NUMBERS: output, every input gradient, dgamma, dbeta, running_mean, running_var and num_batches_tracked against
``F.batch_norm(training=True)`` autograd over the whole batch in f64.  Predicates (``*_ok``) launch nothing and are not recorded.

Tolerances.  f64 comparisons: 1e-9 relative to the largest reference entry -- sums here have fewer than a thousand terms, so f64
rounding stays below 1e-12, while any protocol error (a wrong count, a missing or doubled p_share, local instead of global
statistics) is of order 1 / P >= 1e-3 at these shapes.  Two host functions allocate the weight gradient in f32 whatever the
compute dtype (_concat_resize_conv_grads, _PyramidFuseBNTrain.backward): those two tensors carry ONE f32 rounding of the f64
value, bound 2^-24 relative to the largest entry.  Parameters are drawn as f32-representable doubles because gdlhip.cnn pads
weights and gamma / beta through f32 buffers.  bf16 cases (nodes that require bf16) compare bit for bit against the same
stand-ins composed directly in the test.
"""

import os
import traceback
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F
from torch import nn

from gdlhip import _lib  # noqa: E402
from gdlhip import cnn as gcnn  # noqa: E402
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402

EVAL_MSG = ("gdlhip: autograd through eval-mode BatchNorm is not implemented; call under torch.no_grad() for inference or "
            "model.train() for training")
TOL = 1e-9
TOL_F32_STORE = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ stand-ins
def _acc(x):
    return torch.float64 if x.dtype == torch.float64 else torch.float32


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _put(val, out):
    if out is None:
        return val
    out.copy_(val)
    return out


def _xhat(x, mean, var, eps):
    a = _acc(x)
    return (x.to(a) - mean.to(a)) * torch.rsqrt(var.to(a) + eps)


def _running(rm, rv, mean, var, momentum, count):
    if rm is not None:
        rm.mul_(1 - momentum).add_(mean.to(rm.dtype), alpha=momentum)
        rv.mul_(1 - momentum).add_(var.to(rv.dtype), alpha=momentum * count / max(count - 1, 1))


def _gelu_grad(z):
    return 0.5 * (1 + torch.erf(z * 0.7071067811865476)) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327


class FakeOps:
    """Recording stand-ins for the gdlhip.ops launches of the conv + BatchNorm nodes; ``epilogue_stats`` says whether
    conv_gemm(want_stats=True) delivers partial sums (whole-tile launches on the GPU) or declines (rows == 0)."""

    def __init__(self, epilogue_stats=True):
        self.calls, self.epilogue_stats = [], epilogue_stats

    def install(self, setattr_):
        for name in dir(self):
            if not name.startswith("_") and name not in ("calls", "epilogue_stats", "install"):
                setattr_(ops, name, self._recorded(name))

    def _recorded(self, name):
        fn = getattr(self, name)

        def run(*a, **kw):
            self.calls.append(name)
            return fn(*a, **kw)
        return run

    # ---- operands
    def cast(self, x, dtype, out=None):
        return _put(x.to(dtype), out)

    def copy_cast(self, x, out=None, out_dtype=None):
        return _put(x.to(out_dtype or x.dtype).contiguous(), out)

    def pack_dgrad(self, w, N, T, Cc, out_dtype):
        return w.view(N, T, Cc).flip(1).permute(2, 1, 0).reshape(Cc, T * N).to(out_dtype).contiguous()

    # ---- convolution
    def _conv(self, x, w, R, S, stride, pad, bias=None, resid=None):
        a = _acc(x)
        N, Cc = w.shape[0], x.shape[-1]
        y = F.conv2d(_nchw(x).to(a), w.reshape(N, R, S, Cc).permute(0, 3, 1, 2).to(a), None if bias is None else bias.to(a),
                     stride=stride, padding=pad)
        y = _nhwc(y)
        if resid is not None:
            y = y + resid.to(a)
        return y.to(x.dtype)

    def conv_gemm(self, x, w, *, R=1, S=1, stride=1, pad=0, bias=None, resid=None, out=None, want_stats=False):
        y = _put(self._conv(x, w, R, S, stride, pad, bias, resid), out)
        if not want_stats:
            return y
        if not self.epilogue_stats:
            return y, None, 0
        y2 = y.reshape(-1, y.shape[-1]).float()
        return y, torch.stack([y2.sum(0), (y2 * y2).sum(0)]).unsqueeze(0), 1

    def conv_wgrad(self, x, dy, *, R, S, stride=1, pad=0, dw=None, accumulate=False):
        a = _acc(x)
        N, Cc = dy.shape[-1], x.shape[-1]
        g = torch.nn.grad.conv2d_weight(_nchw(x).to(a), (N, Cc, R, S), _nchw(dy).to(a), stride=stride, padding=pad)
        return _put(g.permute(0, 2, 3, 1).reshape(N, R * S * Cc), dw)

    def convt2x2_pack(self, weight, dtype):
        cin, cout = weight.shape[0], weight.shape[1]
        return (weight.permute(2, 3, 1, 0).reshape(4, cout, cin).to(dtype).contiguous(),
                weight.permute(0, 2, 3, 1).reshape(cin, 4 * cout).to(dtype).contiguous())

    def convt2x2(self, x, w_fwd, bias=None):
        cout, cin = w_fwd.shape[1], w_fwd.shape[2]
        return _nhwc(F.conv_transpose2d(_nchw(x), w_fwd.view(2, 2, cout, cin).permute(3, 2, 0, 1), bias, stride=2))

    def convt2x2_dgrad(self, dy, w_dgrad):
        return self._conv(dy, w_dgrad, 2, 2, 2, 0)

    def convt2x2_wgrad(self, x, dy):
        B, H, W, _ = x.shape
        return torch.einsum("bhwc,bhpwqn->cnpq", x, dy.reshape(B, H, 2, W, 2, dy.shape[-1])).contiguous()

    # ---- BatchNorm (+ ReLU)
    def bn_stats(self, x, running_mean=None, running_var=None, momentum=0.1):
        x2 = x.reshape(-1, x.shape[-1]).to(_acc(x))
        mean, var = x2.mean(0), x2.var(0, unbiased=False)
        _running(running_mean, running_var, mean, var, momentum, x2.shape[0])
        return mean, var

    def bn_stats_finalize(self, partials, rows, channels, pixels, running_mean=None, running_var=None, momentum=0.1):
        s = partials.sum(0)
        mean = s[0] / pixels
        var = (s[1] / pixels - mean * mean).clamp_min(0)
        _running(running_mean, running_var, mean, var, momentum, pixels)
        return mean, var

    def _bn(self, x, mean, var, gamma, beta, eps, relu):
        z = _xhat(x, mean, var, eps) * gamma.to(_acc(x)) + beta.to(_acc(x))
        return (z.clamp_min(0) if relu else z).to(x.dtype)

    def bn_apply(self, x, mean, var, gamma, beta, eps, relu, out=None):
        return _put(self._bn(x, mean, var, gamma, beta, eps, relu), out)

    def _g(self, x, dy, mean, var, gamma, beta, eps, relu):
        """(upstream gradient with the ReLU mask applied, xhat)"""
        a = _acc(x)
        xh = _xhat(x, mean, var, eps)
        g = dy.to(a)
        if relu:
            g = g * (xh * gamma.to(a) + beta.to(a) > 0)
        return g, xh

    def _sums(self, g, xh):
        c = g.shape[-1]
        return (g * xh).reshape(-1, c).sum(0), g.reshape(-1, c).sum(0)

    def _dx(self, x, g, xh, var, gamma, eps, sg, sb, p):
        a = _acc(x)
        return (gamma.to(a) * torch.rsqrt(var.to(a) + eps) * (g - sb.to(a) / p - xh * sg.to(a) / p)).to(x.dtype)

    def bn_bwd_reduce(self, x, dy, mean, var, gamma, beta, eps, relu):
        return self._sums(*self._g(x, dy, mean, var, gamma, beta, eps, relu))

    def bn_bwd_dx(self, x, dy, mean, var, gamma, beta, eps, relu, dgamma_sum, dbeta_sum, p_total, out=None):
        g, xh = self._g(x, dy, mean, var, gamma, beta, eps, relu)
        return _put(self._dx(x, g, xh, var, gamma, eps, dgamma_sum, dbeta_sum, p_total), out)

    def bn_small_fwd(self, x, gamma, beta, eps, relu, running_mean=None, running_var=None, momentum=0.1):
        mean, var = self.bn_stats(x, running_mean, running_var, momentum)
        return self._bn(x, mean, var, gamma, beta, eps, relu), mean, var

    def bn_small_bwd(self, x, dy, mean, var, gamma, beta, eps, relu, out=None):
        g, xh = self._g(x, dy, mean, var, gamma, beta, eps, relu)
        sg, sb = self._sums(g, xh)
        return _put(self._dx(x, g, xh, var, gamma, eps, sg, sb, g.numel() // g.shape[-1]), out), sg, sb

    # ---- BatchNorm -> GELU
    def bn_gelu_apply(self, x, mean, var, gamma, beta, eps, out=None):
        return _put(F.gelu(self._bn(x, mean, var, gamma, beta, eps, False)), out)

    def _g_gelu(self, x, dy, mean, var, gamma, beta, eps):
        xh = _xhat(x, mean, var, eps)
        return dy.to(_acc(x)) * _gelu_grad(xh * gamma + beta), xh

    def bn_gelu_bwd_reduce(self, x, dy, mean, var, gamma, beta, eps):
        return self._sums(*self._g_gelu(x, dy, mean, var, gamma, beta, eps))

    def bn_gelu_bwd_dx(self, x, dy, mean, var, gamma, beta, eps, dgamma_sum, dbeta_sum, p_total, total_count=None, out=None):
        g, xh = self._g_gelu(x, dy, mean, var, gamma, beta, eps)
        p = p_total if total_count is None else total_count
        return _put(self._dx(x, g, xh, var, gamma, eps, dgamma_sum, dbeta_sum, p), out)

    # ---- resampling
    def _up(self, x, size):
        return _nhwc(F.interpolate(_nchw(x).to(_acc(x)), size=tuple(size), mode="bilinear", align_corners=False)).to(x.dtype)

    def bilinear(self, x, size, out=None, out_dtype=None, accumulate=False):
        return _put(self._up(x, size), out)

    def _up_t(self, dout, in_size):
        a = _acc(dout)
        with torch.enable_grad():
            z = torch.zeros(dout.shape[0], dout.shape[-1], *in_size, dtype=a, requires_grad=True)
            up = F.interpolate(z, size=tuple(dout.shape[1:3]), mode="bilinear", align_corners=False)
            (g,) = torch.autograd.grad(up, z, _nchw(dout).to(a))
        return _nhwc(g).to(dout.dtype)

    def bilinear_bwd(self, dout, in_size, din=None, din_dtype=None, accumulate=False):
        return self._up_t(dout, in_size)

    def bilinear_sum(self, xs, size):
        return sum(self._up(x, size) for x in xs)

    def bilinear_add_bn(self, x_pre, mean, var, gamma, beta, eps, relu, x):
        a = _acc(x_pre)
        z = self._bn(x_pre, mean, var, gamma, beta, eps, relu)
        return (z.to(a) + self._up(x, x_pre.shape[1:3]).to(a)).to(x_pre.dtype)

    def resize_conv3x3_bwd(self, x_lo, dy, w_dgrad, want_dw=True, g=None):
        dx = None if w_dgrad is None else self._up_t(self._conv(dy, w_dgrad, 3, 3, 1, 1), x_lo.shape[1:3])
        dw = self.conv_wgrad(self._up(x_lo, dy.shape[1:3]), dy, R=3, S=3, pad=1) if want_dw else None
        return dx, dw


class _FakeLib:
    """The shape predicates the nodes ask the library directly: every shape of this file is accepted."""

    def __getattr__(self, name):
        if name.endswith("_ok"):
            return lambda *a: 1
        raise AttributeError(name)


@pytest.fixture
def fake(monkeypatch):
    f = FakeOps()
    f.install(monkeypatch.setattr)
    monkeypatch.setattr(_lib, "load", lambda: _FakeLib())
    monkeypatch.setattr(gnn, "SYNC_MESSAGES", [0, 0])
    return f


# ------------------------------------------------------------------------------------------------ inputs, reference, checks
def _rand(gen, *shape, dtype=torch.float64):
    """f32-representable values in the requested dtype"""
    return torch.randn(*shape, generator=gen, dtype=torch.float32).to(dtype)


def _init(gen, *modules):
    for m in modules:
        for name, p in list(m.named_parameters()) + [(n, b) for n, b in m.named_buffers() if b.is_floating_point()]:
            with torch.no_grad():
                v = _rand(gen, *p.shape) * 0.3
                if name == "running_var" or (isinstance(m, nn.modules.batchnorm._NormBase) and name == "weight"):
                    v = v.abs() + 0.5
                p.copy_(v.float())
    return modules


def _ref_bn(y, norm, act):
    """F.batch_norm(training=True) on NCHW y with clones of the module's parameters / buffers -> (out, gamma, beta, rm, rv)"""
    gamma, beta = norm.weight.detach().clone().requires_grad_(), norm.bias.detach().clone().requires_grad_()
    rm, rv = norm.running_mean.clone(), norm.running_var.clone()
    z = F.batch_norm(y, rm, rv, gamma, beta, True, norm.momentum, norm.eps)
    z = {"relu": F.relu, "gelu": F.gelu, "none": lambda t: t}[act](z)
    return z, gamma, beta, rm, rv


def _close(got, want, what, tol=TOL):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got.double() - want.double()).abs().max().item() / max(want.double().abs().max().item(), 1e-300)
    assert err <= tol, f"{what}: relative error {err:.3e} > {tol:.1e}"


def _check_norm(norm, gamma, beta, rm, rv, what, rows=slice(None)):
    _close(norm.weight.grad, gamma.grad[rows], f"{what} dgamma")
    _close(norm.bias.grad, beta.grad[rows], f"{what} dbeta")
    _close(norm.running_mean, rm, f"{what} running_mean")
    _close(norm.running_var, rv, f"{what} running_var")
    assert int(norm.num_batches_tracked) == 1, what


def _leaf(t):
    return t.detach().clone().requires_grad_()


# ------------------------------------------------------------------------------------------------ 1. conv_bn_act, single process
CBA_FWD = ["cast", "conv_gemm", "bn_stats", "bn_apply"]
CBA_BWD = ["bn_bwd_reduce", "bn_bwd_dx", "pack_dgrad", "conv_gemm", "conv_wgrad"]


def _conv_bn_act_case(gen, x_full, rows, norm_cls, *, relu=True, bias=False):
    """Runs gnn.conv_bn_act on x_full[rows] and returns what the checks need next to the whole-batch reference."""
    conv, norm = _init(gen, nn.Conv2d(8, 8, 3, padding=1, bias=bias).double(), norm_cls(8).double())
    G = _rand(gen, x_full.shape[0], 6, 6, 8)
    xr, wr = _leaf(x_full), _leaf(conv.weight)
    br = _leaf(conv.bias) if bias else None
    ref, gamma, beta, rm, rv = _ref_bn(F.conv2d(_nchw(xr), wr, br, padding=1), norm, "relu" if relu else "none")
    ref = ref.permute(0, 2, 3, 1)
    (ref * G).sum().backward()
    x = _leaf(x_full[rows])
    out = gnn.conv_bn_act(x, conv, norm, relu=relu)
    (out * G[rows]).sum().backward()
    return dict(conv=conv, norm=norm, x=x, out=out, ref=ref, xr=xr, wr=wr, gamma=gamma, beta=beta, rm=rm, rv=rv)


@pytest.mark.parametrize("variant", ["plain", "no_relu", "bias", "small_map"])
def test_conv_bn_act_single_process(fake, monkeypatch, variant):
    gen = torch.Generator().manual_seed(11)
    if variant == "small_map":
        monkeypatch.setattr(ops, "BN_SMALL_MAX_PIXELS", 1000)
    r = _conv_bn_act_case(gen, _rand(gen, 2, 6, 6, 8), slice(None), nn.BatchNorm2d, relu=variant != "no_relu", bias=variant == "bias")
    if variant == "small_map":
        assert fake.calls == ["cast", "conv_gemm", "bn_small_fwd", "bn_small_bwd", "pack_dgrad", "conv_gemm", "conv_wgrad"]
    else:
        assert fake.calls == CBA_FWD + CBA_BWD
    assert gnn.SYNC_MESSAGES == [0, 0]
    _close(r["out"], r["ref"], "out")
    _close(r["x"].grad, r["xr"].grad, "dx")
    _close(r["conv"].weight.grad, r["wr"].grad, "dw")
    _check_norm(r["norm"], r["gamma"], r["beta"], r["rm"], r["rv"], variant)
    if variant == "bias":      # a bias feeding train-mode BatchNorm: exact zeros, not a rounding residue
        assert r["conv"].bias.grad.shape == (8,) and torch.count_nonzero(r["conv"].bias.grad) == 0


def _bf16_lateral(gen):
    conv, norm = _init(gen, nn.Conv2d(8, 8, 1), nn.BatchNorm2d(8))
    x = _rand(gen, 2, 6, 6, 8, dtype=torch.bfloat16)
    return conv, norm, x


def _bf16_expected(e, conv, norm, x, producer, tail):
    """The protocol composed from the stand-ins directly (bf16 nodes): returns (y, mean, var, rm, rv, g, b) and the forward
    result of ``tail(y, mean, var, g, b)``."""
    w = conv.weight.detach().permute(0, 2, 3, 1).reshape(8, -1).to(torch.bfloat16)
    rm, rv = norm.running_mean.clone(), norm.running_var.clone()
    if producer:
        y, part, rows = e.conv_gemm(x.detach(), w, bias=conv.bias.detach(), want_stats=True)
        mean, var = e.bn_stats_finalize(part, rows, 8, y.numel() // 8, rm, rv, norm.momentum)
    else:
        y = e.conv_gemm(x.detach(), w, bias=conv.bias.detach())
        mean, var = e.bn_stats(y, rm, rv, norm.momentum)
    g, b = norm.weight.detach(), norm.bias.detach()
    return y, mean, var, rm, rv, g, b, w, tail(y, mean, var, g, b)


def _bf16_check_backward(e, conv, norm, x, y, mean, var, g, b, w, gout, rm, rv):
    sg, sb = e.bn_bwd_reduce(y, gout, mean, var, g, b, norm.eps, True)
    dy = e.bn_bwd_dx(y, gout, mean, var, g, b, norm.eps, True, sg, sb, y.numel() // 8)
    dx = e.conv_gemm(dy, e.pack_dgrad(conv.weight.detach().permute(0, 2, 3, 1).reshape(8, -1).contiguous(), 8, 1, 8, torch.bfloat16))
    dw = e.conv_wgrad(x.detach(), dy, R=1, S=1).view(8, 8, 1, 1)
    for got, want in ((x.grad, dx), (conv.weight.grad, dw), (norm.weight.grad, sg), (norm.bias.grad, sb),
                      (norm.running_mean, rm), (norm.running_var, rv)):
        torch.testing.assert_close(got, want.to(got.dtype), rtol=0, atol=0)
    assert torch.count_nonzero(conv.bias.grad) == 0 and int(norm.num_batches_tracked) == 1


def test_conv_bn_act_statistics_delivered_by_the_producer(fake):
    """bf16: the convolution's epilogue emits the partial sums, no statistics pass runs, the producer's finalize kernel has
    written the running buffers."""
    gen = torch.Generator().manual_seed(12)
    conv, norm, x = _bf16_lateral(gen)
    e = FakeOps()
    y, mean, var, rm, rv, g, b, w, want = _bf16_expected(e, conv, norm, x, True, lambda y, m, v, g, b: e.bn_apply(y, m, v, g, b, norm.eps, True))
    G = _rand(gen, 2, 6, 6, 8, dtype=torch.bfloat16)
    x.requires_grad_()
    out = gnn.conv_bn_act(x, conv, norm)
    (out.float() * G.float()).sum().backward()
    assert fake.calls == ["cast", "conv_gemm", "bn_stats_finalize", "bn_apply"] + CBA_BWD
    assert gnn.SYNC_MESSAGES == [0, 0]
    torch.testing.assert_close(out, want, rtol=0, atol=0)
    _bf16_check_backward(e, conv, norm, x, y, mean, var, g, b, w, G, rm, rv)


# ------------------------------------------------------------------------------------------------ 2. the other nodes, single process
def test_concat_resize_conv_bn_act_concat_buffer_branch(fake, monkeypatch):
    monkeypatch.setattr(gnn, "FUSE_TAPSUM", False)
    gen = torch.Generator().manual_seed(21)
    conv, norm = _init(gen, nn.Conv2d(16, 8, 3, padding=1, bias=False).double(), nn.BatchNorm2d(8).double())
    l0, l1, G = _rand(gen, 2, 6, 6, 8), _rand(gen, 2, 3, 3, 8), _rand(gen, 2, 6, 6, 8)
    r0, r1, wr = _leaf(l0), _leaf(l1), _leaf(conv.weight)
    cat = torch.cat([_nchw(r0), F.interpolate(_nchw(r1), size=(6, 6), mode="bilinear", align_corners=False)], 1)
    ref, gamma, beta, rm, rv = _ref_bn(F.conv2d(cat, wr, padding=1), norm, "relu")
    (ref.permute(0, 2, 3, 1) * G).sum().backward()
    a0, a1 = _leaf(l0), _leaf(l1)
    out = gnn.concat_resize_conv_bn_act([a0, a1], conv, norm)
    (out * G).sum().backward()
    assert fake.calls == ["bilinear", "bilinear", "cast", "conv_gemm", "bn_stats", "bn_apply",
                          "bn_bwd_reduce", "bn_bwd_dx", "pack_dgrad", "conv_gemm", "conv_wgrad", "resize_conv3x3_bwd"]
    assert gnn.SYNC_MESSAGES == [0, 0]
    _close(out, ref.permute(0, 2, 3, 1), "out")
    _close(a0.grad, r0.grad, "d level 0")
    _close(a1.grad, r1.grad, "d level 1")
    _close(conv.weight.grad, wr.grad, "dw", TOL_F32_STORE)
    _check_norm(norm, gamma, beta, rm, rv, "concat")


def test_pyramid_fuse_bn_act(fake):
    gen = torch.Generator().manual_seed(22)
    conv, norm = _init(gen, nn.Conv2d(16, 8, 1, bias=False).double(), nn.BatchNorm2d(8).double())
    l0, l1, G = _rand(gen, 2, 3, 3, 8), _rand(gen, 2, 6, 6, 8), _rand(gen, 2, 6, 6, 8)
    r0, r1, wr = _leaf(l0), _leaf(l1), _leaf(conv.weight)
    cat = torch.cat([F.interpolate(_nchw(r0), size=(6, 6), mode="bilinear", align_corners=False), _nchw(r1)], 1)
    ref, gamma, beta, rm, rv = _ref_bn(F.conv2d(cat, wr), norm, "relu")
    (ref.permute(0, 2, 3, 1) * G).sum().backward()
    a0, a1 = _leaf(l0), _leaf(l1)
    out = gnn.pyramid_fuse_bn_act([a0, a1], conv, norm)
    (out * G).sum().backward()
    assert fake.calls == ["cast", "conv_gemm", "bilinear_sum", "conv_gemm", "bn_stats", "bn_apply",
                          "bn_bwd_reduce", "bn_bwd_dx", "bilinear_bwd", "pack_dgrad", "conv_gemm", "conv_gemm", "conv_wgrad", "conv_wgrad"]
    assert gnn.SYNC_MESSAGES == [0, 0]
    _close(out, ref.permute(0, 2, 3, 1), "out")
    _close(a0.grad, r0.grad, "d level 0")
    _close(a1.grad, r1.grad, "d level 1")
    _close(conv.weight.grad, wr.grad, "dw", TOL_F32_STORE)
    _check_norm(norm, gamma, beta, rm, rv, "pyramid")


CONVT_CALLS = ["convt2x2_pack", "convt2x2", "bn_stats", "bn_gelu_apply",
               "bn_gelu_bwd_reduce", "bn_gelu_bwd_dx", "convt2x2_dgrad", "convt2x2_wgrad"]


def _convt_case(gen, x_full, rows, norm_cls):
    convt, norm = _init(gen, nn.ConvTranspose2d(8, 8, 2, stride=2).double(), norm_cls(8).double())
    G = _rand(gen, x_full.shape[0], 12, 12, 8)
    xr, wr, br = _leaf(x_full), _leaf(convt.weight), _leaf(convt.bias)
    ref, gamma, beta, rm, rv = _ref_bn(F.conv_transpose2d(_nchw(xr), wr, br, stride=2), norm, "gelu")
    ref = ref.permute(0, 2, 3, 1)
    (ref * G).sum().backward()
    x = _leaf(x_full[rows])
    out = gnn.conv_transpose2x2_bn_gelu(x, convt, norm)
    (out * G[rows]).sum().backward()
    return dict(conv=convt, norm=norm, x=x, out=out, ref=ref, xr=xr, wr=wr, gamma=gamma, beta=beta, rm=rm, rv=rv)


def test_conv_transpose2x2_bn_gelu(fake):
    gen = torch.Generator().manual_seed(23)
    r = _convt_case(gen, _rand(gen, 2, 6, 6, 8), slice(None), nn.BatchNorm2d)
    assert fake.calls == CONVT_CALLS
    assert gnn.SYNC_MESSAGES == [0, 0]
    _close(r["out"], r["ref"], "out")
    _close(r["x"].grad, r["xr"].grad, "dx")
    _close(r["conv"].weight.grad, r["wr"].grad, "dw")
    assert torch.count_nonzero(r["conv"].bias.grad) == 0
    _check_norm(r["norm"], r["gamma"], r["beta"], r["rm"], r["rv"], "convt")


@pytest.mark.parametrize("producer", [False, True], ids=["statistics_pass", "producer_statistics"])
def test_conv_bn_act_upsample_add_fused_branch(fake, producer):
    """bf16 (the node requires it): ReLU(BN(conv1x1(x))) + bilinear(b) without the normalised lateral."""
    fake.epilogue_stats = producer
    gen = torch.Generator().manual_seed(24)
    conv, norm, x = _bf16_lateral(gen)
    b_in = _rand(gen, 2, 3, 3, 8, dtype=torch.bfloat16)
    e = FakeOps(producer)
    y, mean, var, rm, rv, g, b, w, want = _bf16_expected(
        e, conv, norm, x, producer, lambda y, m, v, g, b: e.bilinear_add_bn(y, m, v, g, b, norm.eps, True, b_in))
    G = _rand(gen, 2, 6, 6, 8, dtype=torch.bfloat16)
    x.requires_grad_()
    b_leaf = b_in.clone().requires_grad_()
    out = gnn.conv_bn_act_upsample_add(x, conv, norm, b_leaf)
    (out.float() * G.float()).sum().backward()
    assert fake.calls == ["cast", "conv_gemm", "bn_stats_finalize" if producer else "bn_stats", "bilinear_add_bn", "bilinear_bwd"] + CBA_BWD
    assert gnn.SYNC_MESSAGES == [0, 0]
    torch.testing.assert_close(out, want, rtol=0, atol=0)
    torch.testing.assert_close(b_leaf.grad, e.bilinear_bwd(G, (3, 3)), rtol=0, atol=0)
    _bf16_check_backward(e, conv, norm, x, y, mean, var, g, b, w, G, rm, rv)


CNN_CALLS = ["cast", "pack_dgrad", "conv_gemm", "bn_stats", "bn_apply", "bn_bwd_reduce", "bn_bwd_dx", "conv_wgrad", "conv_gemm"]


def _cnn_case(gen, x_full, rows, norm_cls, n):
    norm, = _init(gen, norm_cls(n).double())
    weight = nn.Parameter((_rand(gen, n, 8, 3, 3) * 0.3).float().double())
    G = _rand(gen, x_full.shape[0], 6, 6, 8)
    xr, wr = _leaf(x_full), _leaf(weight)
    ref, gamma, beta, rm, rv = _ref_bn(F.conv2d(_nchw(xr), wr, padding=1), norm, "relu")
    ref = ref.permute(0, 2, 3, 1)
    (ref * G[..., :n]).sum().backward()
    x = _leaf(x_full[rows])
    out = gcnn.conv_bn(x, weight, norm, pad=1)
    (out * G[rows]).sum().backward()
    return dict(conv=SimpleNamespace(weight=weight), norm=norm, x=x, out=out, ref=ref, xr=xr, wr=wr, gamma=gamma, beta=beta,
                rm=rm, rv=rv, n=n)


def _check_cnn(r, ref_rows, what):
    n = r["n"]
    assert r["out"].shape[-1] == 8 and torch.count_nonzero(r["out"][..., n:]) == 0      # padded channels: exactly zero
    _close(r["out"][..., :n], r["ref"][ref_rows], f"{what} out")
    _close(r["x"].grad, r["xr"].grad[ref_rows], f"{what} dx")
    assert r["norm"].weight.grad.shape == (n,) and r["norm"].bias.grad.shape == (n,)     # cut back from the padded width


@pytest.mark.parametrize("n", [8, 6], ids=["n_eq_npad", "n_lt_npad"])
def test_cnn_conv_bn(fake, n):
    gen = torch.Generator().manual_seed(25)
    r = _cnn_case(gen, _rand(gen, 2, 6, 6, 8), slice(None), nn.BatchNorm2d, n)
    assert fake.calls == CNN_CALLS
    assert gnn.SYNC_MESSAGES == [0, 0]
    _check_cnn(r, slice(None), "cnn")
    _close(r["conv"].weight.grad, r["wr"].grad, "dw")
    _check_norm(r["norm"], r["gamma"], r["beta"], r["rm"], r["rv"], "cnn")


# ------------------------------------------------------------------------------------------------ 3. two ranks, ragged 1 + 2 images
def test_ragged_split_tells_per_rank_statistics_from_global_ones():
    """The condition the two-rank cases rest on: with 1 + 2 images the whole-batch reference and a per-rank BatchNorm differ by
    far more than the tolerance (with equal counts a mean of per-rank means would equal the global mean)."""
    gen = torch.Generator().manual_seed(31)
    x = _rand(gen, 3, 6, 6, 8)
    conv, norm = _init(gen, nn.Conv2d(8, 8, 3, padding=1, bias=False).double(), nn.BatchNorm2d(8).double())
    y = F.conv2d(_nchw(x), conv.weight, padding=1)
    whole = _ref_bn(y, norm, "none")[0]
    per_rank = torch.cat([_ref_bn(y[:1], norm, "none")[0], _ref_bn(y[1:], norm, "none")[0]])
    assert ((whole - per_rank).abs().max() / whole.abs().max()).item() > 1e3 * TOL
    assert ((y.mean((0, 2, 3)) - (y[:1].mean((0, 2, 3)) + y[1:].mean((0, 2, 3))) / 2).abs().max() / y.abs().max()).item() > 1e3 * TOL


def _reduced(t):
    t = t.detach().clone()
    dist.all_reduce(t)
    return t


def _rank_case_conv_bn_act(fake, rows):
    gen = torch.Generator().manual_seed(32)
    r = _conv_bn_act_case(gen, _rand(gen, 3, 6, 6, 8), rows, nn.SyncBatchNorm)
    assert fake.calls == CBA_FWD + CBA_BWD, fake.calls
    _close(r["out"], r["ref"][rows], "out")
    _close(r["x"].grad, r["xr"].grad[rows], "dx")
    _close(_reduced(r["conv"].weight.grad), r["wr"].grad, "dw")
    return r


def _rank_case_convt(fake, rows):
    gen = torch.Generator().manual_seed(33)
    r = _convt_case(gen, _rand(gen, 3, 6, 6, 8), rows, nn.SyncBatchNorm)
    assert fake.calls == CONVT_CALLS, fake.calls
    _close(r["out"], r["ref"][rows], "out")
    _close(r["x"].grad, r["xr"].grad[rows], "dx")
    _close(_reduced(r["conv"].weight.grad), r["wr"].grad, "dw")
    assert torch.count_nonzero(r["conv"].bias.grad) == 0
    return r


def _rank_case_cnn(fake, rows):
    gen = torch.Generator().manual_seed(34)
    r = _cnn_case(gen, _rand(gen, 3, 6, 6, 8), rows, nn.SyncBatchNorm, 6)
    assert fake.calls == CNN_CALLS, fake.calls
    _check_cnn(r, rows, "cnn")
    _close(_reduced(r["conv"].weight.grad), r["wr"].grad, "dw")
    return r


def _rank_case_group(fake, rows):
    """Two members (3x3 and 1x1 ConvModules on different inputs): ONE message each way for both."""
    gen = torch.Generator().manual_seed(35)
    xs = [_rand(gen, 3, 6, 6, 8), _rand(gen, 3, 6, 6, 8)]
    Gs = [_rand(gen, 3, 6, 6, 8), _rand(gen, 3, 6, 6, 8)]
    convs = [nn.Conv2d(8, 8, 3, padding=1, bias=False).double(), nn.Conv2d(8, 8, 1).double()]
    norms = [nn.SyncBatchNorm(8).double(), nn.SyncBatchNorm(8).double()]
    _init(gen, *convs, *norms)
    refs = []
    for x_full, G, conv, norm in zip(xs, Gs, convs, norms):
        xr, wr = _leaf(x_full), _leaf(conv.weight)
        ref, gamma, beta, rm, rv = _ref_bn(F.conv2d(_nchw(xr), wr, None if conv.bias is None else conv.bias.detach(), padding=conv.padding), norm, "relu")
        ref = ref.permute(0, 2, 3, 1)
        (ref * G).sum().backward()
        refs.append(dict(ref=ref, xr=xr, wr=wr, gamma=gamma, beta=beta, rm=rm, rv=rv))
    mine = [_leaf(x_full[rows]) for x_full in xs]
    outs = gnn.conv_bn_act_group([dict(x=x, conv=c, norm=nm) for x, c, nm in zip(mine, convs, norms)])
    sum((o * G[rows]).sum() for o, G in zip(outs, Gs)).backward()
    member_fwd, member_bwd = ["cast", "conv_gemm", "bn_stats"], ["bn_bwd_dx", "pack_dgrad", "conv_gemm", "conv_wgrad"]
    assert fake.calls == member_fwd * 2 + ["bn_apply"] * 2 + ["bn_bwd_reduce"] * 2 + member_bwd * 2, fake.calls
    assert gnn.SYNC_MESSAGES == [1, 1], gnn.SYNC_MESSAGES
    for i, (x, out, conv, norm, r) in enumerate(zip(mine, outs, convs, norms, refs)):
        _close(out, r["ref"][rows], f"member {i} out")
        _close(x.grad, r["xr"].grad[rows], f"member {i} dx")
        _close(_reduced(conv.weight.grad), r["wr"].grad, f"member {i} dw")
        norm.weight.grad, norm.bias.grad = _reduced(norm.weight.grad), _reduced(norm.bias.grad)
        _check_norm(norm, r["gamma"], r["beta"], r["rm"], r["rv"], f"member {i}")
    assert torch.count_nonzero(convs[1].bias.grad) == 0
    return None


RANK_CASES = {"conv_bn_act": _rank_case_conv_bn_act, "conv_transpose2x2_bn_gelu": _rank_case_convt,
              "cnn_conv_bn_padded": _rank_case_cnn, "conv_bn_act_group": _rank_case_group}


def _rank_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _lib.load = lambda: _FakeLib()
        rows = slice(0, 1) if rank == 0 else slice(1, 3)
        verdicts = {}
        for name, case in RANK_CASES.items():
            fake = FakeOps()
            fake.install(setattr)
            gnn.SYNC_MESSAGES[:] = [0, 0]
            failed = None
            try:      # (a failing rank still answers its peer's collectives of the later cases)
                r = case(fake, rows)
                if r is not None:
                    assert gnn.SYNC_MESSAGES == [1, 1], gnn.SYNC_MESSAGES
            except Exception:
                failed, r = traceback.format_exc(), None
            try:
                if r is not None:      # parameter gradients of the norm: summed over the ranks like DDP would
                    r["norm"].weight.grad, r["norm"].bias.grad = _reduced(r["norm"].weight.grad), _reduced(r["norm"].bias.grad)
                    _check_norm(r["norm"], r["gamma"], r["beta"], r["rm"], r["rv"], name, slice(0, r.get("n", 8)))
            except Exception:
                failed = traceback.format_exc()
            verdicts[name] = failed or "ok"
            if failed:
                break
        ret[rank] = verdicts
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks():
    """One pair of spawned gloo processes runs all four two-rank cases; every test below reads its own verdicts."""
    world, port = 2, 29500 + (os.getpid() + 13) % 2000
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
    return [p.exitcode for p in procs], {r: ret.get(r) for r in range(world)}


@pytest.mark.parametrize("name", list(RANK_CASES))
def test_two_ranks_ragged_batch(two_ranks, name):
    """World size 2 over gloo, CPU tensors (the torch-built message path), rank 0 holds 1 image and rank 1 holds 2: one message
    per direction and node, running buffers equal to torch's for the FULL batch, every rank's output / dx equal to its slice of
    the full-batch reference, parameter gradients summing to the full-batch ones."""
    codes, verdicts = two_ranks
    assert codes == [0, 0], (codes, verdicts)
    for rank in (0, 1):
        assert verdicts[rank] is not None and verdicts[rank].get(name) == "ok", f"rank {rank}: {verdicts[rank]}"


# ------------------------------------------------------------------------------------------------ 4. eval-mode refusals
def test_eval_mode_refusals_share_one_text(fake):
    conv3, conv1 = nn.Conv2d(8, 8, 3, padding=1, bias=False).double(), nn.Conv2d(16, 8, 1, bias=False).double()
    convt, norm = nn.ConvTranspose2d(8, 8, 2, stride=2).double(), nn.BatchNorm2d(8).double().eval()
    x, lo = torch.zeros(2, 6, 6, 8, dtype=torch.float64), torch.zeros(2, 3, 3, 8, dtype=torch.float64)
    sites = [lambda: gnn.conv_bn_act(x, conv3, norm),
             lambda: gnn.pyramid_fuse_bn_act([lo, x], conv1, norm),
             lambda: gnn.conv_transpose2x2_bn_gelu(x, convt, norm),
             lambda: gcnn.conv_bn(x, conv3.weight, norm, pad=1)]
    for site in sites:
        with pytest.raises(NotImplementedError) as info:
            site()
        assert str(info.value) == EVAL_MSG
