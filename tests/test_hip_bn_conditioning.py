"""Train-mode BatchNorm on ill-conditioned inputs: every producer of batch statistics, and every kernel that consumes them, on a
ladder of kappa = |mean| / std in {0.25, 30, 300, 1000}, once with std = 1 and once with std = 0.01 (where eps = 1e-5 matters).

Reference: f64 BatchNorm (forward and autograd) of the exact STORED input values (quantised to the storage dtype first, then
widened).  torch's own f32 F.batch_norm runs on the same tensor: its error against f64 is the yardstick of the outputs and
gradients (a kernel may be 4 x that -- another summation order -- plus one rounding of its output dtype; y is capped by what
f32-rounded statistics can cost, y_cap), and torch's f32 x.var() must itself meet the variance bound (the bound is one an f32
implementation can meet).

Bounds (none of them comes from what the kernels give):
  variance   |v - v64| <= 1e-5 (v64 + eps): one-pass f32 sums about a pivot within a few std of the mean behave like kappa ~ 10
             of the plain one-pass formula (2e-6 relative); 5 x that, 100 x torch's f32 error.
  mean       2 f32 ulps of |mean| + 1e-6 std.
  running    the same scaled by the momentum, plus one f32 ulp of the stored buffer value (the buffer is f32: a correctly rounded
             update is half an ulp off, an update evaluated in f32 up to one and a half).
  fused producers (GEMM epilogue, resized-conv forward sums): plain sums of x and x^2 in f32 -- see FUSED_* below.

Every case prints its measured figures (`BNCOND ...` lines; DESIGN.md section 3 tabulates them)."""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402

DEV = "cuda"
EPS, MOM = 1e-5, 0.1
RUNGS = (0.25, 30.0, 300.0, 1000.0)
SCALES = (1.0, 0.01)
DTYPES = (torch.float32, torch.bfloat16)
VAR_TOL = 1e-5
# one round-to-nearest into the output dtype, relative to the value: 2^-p for a p-bit significand (f32: 24, bf16: 8)
ROUNDING = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}
STATS_SHAPES = [(2, 9, 7, 64), (2, 31, 9, 32),             # generic kernels
                (1, 64, 64, 64), (2, 48, 48, 96)]          # >= 4096 pixels: the bf16 backward sums take the 16-byte-load kernels
SMALL_SHAPES = [(2, 3, 3, 768), (3, 37, 5, 12), (1, 45, 91, 16)]


def ulp32(t):
    """one f32 ulp of |t| (t: f64 tensor)"""
    a = t.abs().float().clamp_min(1e-38)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def kappa_floor(rung, dtype):
    """kappa a tensor built for `rung` must still have once stored: bf16's 8-bit mantissa adds a quantisation variance of up to
    (|mean| 2^-7)^2 / 12, which caps kappa near 890; 0.9 covers the difference between that model and the sample."""
    if dtype == torch.bfloat16:
        rung = 1.0 / math.sqrt(1.0 / rung ** 2 + 2.0 ** -14 / 12)
    return 0.9 * rung


def _seed(*key):
    h = 17
    for k in key:
        for ch in repr(k):
            h = (h * 131 + ord(ch)) % 2147483629
    return h


def case(shape, rung, std, dtype, sign=1, special="", act="none"):
    """One input tensor and its f64 reference (CPU; milliseconds at these shapes, so nothing is kept between cases)."""
    B, H, W, C = shape
    P = B * H * W
    g = torch.Generator().manual_seed(_seed(shape, rung, std, dtype, sign, special))
    z = torch.randn(P, C, generator=g, dtype=torch.float64)
    if P > 2:      # the sample itself has mean 0 and std 1: the channel sits ON its rung, not near it
        z = (z - z.mean(0)) / z.std(0, unbiased=False)
    kap = torch.full((C,), float(rung), dtype=torch.float64)
    if special == "mixed":                   # one kappa = 1000 channel inside a 4- and an 8-channel lane group of kappa = 0.25 neighbours
        kap[:] = 0.25
        kap[5] = 1000.0
    x = z * std + sign * kap * std
    if special == "const":
        x[:, 2] = 1000.125
    x = x.float().to(dtype).float().reshape(B, H, W, C)           # the stored values, exactly
    r = dict(P=P, C=C, x=x, std=std, rung=rung)
    r["gamma"], r["beta"] = torch.randn(C, generator=g), torch.randn(C, generator=g)
    r["rm0"], r["rv0"] = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g).abs() + 0.5
    r["dy"] = torch.randn(B, H, W, C, generator=g).to(dtype).float()
    x64 = x.double().reshape(P, C)
    m, v = x64.mean(0), x64.var(0, unbiased=False)
    r["mean"], r["var"] = m, v
    r["kappa"] = m.abs() / v.sqrt().clamp_min(1e-300)
    r["rm"] = (1 - MOM) * r["rm0"].double() + MOM * m
    r["rv"] = (1 - MOM) * r["rv0"].double() + MOM * (v * P / (P - 1) if P > 1 else v)
    if P == 1:          # torch refuses one value per channel in training: statistics only
        return r

    def run(dt):
        xr = x.to(dt).permute(0, 3, 1, 2).clone().requires_grad_(True)
        gr, br = r["gamma"].to(dt).requires_grad_(True), r["beta"].to(dt).requires_grad_(True)
        rm_t, rv_t = torch.zeros(C, dtype=dt), torch.zeros(C, dtype=dt)
        pre = F.batch_norm(xr, rm_t, rv_t, gr, br, True, 1.0, EPS)          # momentum 1: running_var = the unbiased batch variance
        y = F.relu(pre) if act == "relu" else (F.gelu(pre) if act == "gelu" else pre)
        y.backward(r["dy"].to(dt).permute(0, 3, 1, 2))
        nhwc = lambda t: t.detach().permute(0, 2, 3, 1).double()          # noqa: E731
        return dict(y=nhwc(y), dx=nhwc(xr.grad), dg=gr.grad.double(), db=br.grad.double(), pre=nhwc(pre), var=rv_t.double() * (P - 1) / P)

    ref, t32 = run(torch.float64), run(torch.float32)
    r.update({k: t for k, t in ref.items() if k != "var"})
    # channels the ReLU cases leave out (rule of test_batchnorm_small_map_single_launch): an f64 pre-activation within 1e-4 of zero
    r["ok"] = (ref["pre"].abs() >= 1e-4).reshape(P, C).all(0) if act == "relu" else torch.ones(C, dtype=torch.bool)
    if act == "relu":
        assert int(r["ok"].sum()) >= C // 2, "too few channels left to compare: choose another seed"
    ok = r["ok"]
    r["torch_err"] = {k: ((t32[k] - ref[k])[..., ok].abs().max() / ref[k][..., ok].abs().max().clamp_min(1e-300)).item()
                      for k in ("y", "dx", "dg", "db")}
    # torch's f32 yardsticks of the variance: x.var() (two-pass, pairwise sums) is the one the bound is checked against;
    # the variance F.batch_norm's CPU kernel itself forms adds P terms per thread in f32 and lands anywhere between 4e-7 and
    # 7e-5 at 4608 pixels, depending on the number of threads -- printed, not asserted
    v32 = x.reshape(P, C).var(0, unbiased=False).double()
    r["torch_var_err"] = ((v32 - v).abs() / (v + EPS)).max().item()
    r["torch_bn_var_err"] = ((t32["var"] - v).abs() / (v + EPS)).max().item()
    return r


def assert_reached(r, dtype, what, rung=None):
    rung = r["rung"] if rung is None else rung
    reached = (r["kappa"] >= kappa_floor(rung, dtype)).double().mean().item()
    assert reached >= 0.75, f"{what}: only {reached:.0%} of the channels reached kappa {rung} (median {r['kappa'].median().item():.3g})"


def check_stats(r, mean, var, rm, rv, what, running_var=True, var_tol=VAR_TOL, input_term=0.0):
    """mean / var / running buffers of a producer against the f64 statistics, every channel.  ``input_term``: what the rounding of
    the producer's INPUTS alone moves the variance by (per channel, absolute), where a case has such a term."""
    m64, v64 = r["mean"], r["var"]
    mean, var = mean.double().cpu(), var.double().cpu()
    ev = (((var - v64).abs() - input_term).clamp_min(0) / (v64 + EPS)).max().item()
    tol_m = 2 * ulp32(m64) + 1e-6 * v64.sqrt()
    em = ((mean - m64).abs() / tol_m).max().item()
    line = f"BNCOND {what} kappa={r['kappa'].median().item():.4g} var_err={ev:.3e} (torch f32 var() {r.get('torch_var_err', float('nan')):.1e}, F.batch_norm {r.get('torch_bn_var_err', float('nan')):.1e}) mean_err/tol={em:.3f}"
    erm = erv = 0.0
    if rm is not None:
        erm = ((rm.double().cpu() - r["rm"]).abs() / (MOM * tol_m + ulp32(r["rm"]))).max().item()
        erv = ((rv.double().cpu() - r["rv"]).abs() / (MOM * var_tol * (v64 + EPS) + ulp32(r["rv"]))).max().item() if running_var else 0.0
        line += f" running_mean_err/tol={erm:.3f} running_var_err/tol={erv:.3f}"
    print(line)
    assert torch.isfinite(mean).all() and torch.isfinite(var).all() and (var >= 0).all(), what
    assert ev <= var_tol, f"{what}: variance off by {ev:.3e} (v + eps)"
    assert em <= 1.0, f"{what}: mean off by {em:.3f} x (2 ulp + 1e-6 std)"
    assert erm <= 1.0 and erv <= 1.0, f"{what}: running buffers off by {erm:.3f} / {erv:.3f} x their bound"
    return ev


def y_cap(r, fed):
    """What an evaluation of gamma (x - mean) rstd + beta in f32 can owe to its statistics, relative to max |y|: torch's own f32
    error grows with kappa (its CPU kernel forms x alpha + (beta - mean alpha), which rounds at the size of kappa), so 4 x torch
    alone would let that very form pass on the upper rungs.  First order: |gamma| dmean / sqrt(v + eps) (x 1.13 = max |gelu'|) with
    dmean = half an f32 ulp of the mean when the kernel is FED the rounded reference mean, the mean bound for a producer's own
    statistics; half the relative variance error (2^-24 fed, the 1e-5 bound own); eight f32 roundings for the expression itself."""
    ok = r["ok"]
    m64, v64 = r["mean"][ok], r["var"][ok]
    dmean = ulp32(m64) / 2 if fed else 2 * ulp32(m64) + 1e-6 * v64.sqrt()
    first = (1.13 * r["gamma"][ok].double().abs() * dmean / (v64 + EPS).sqrt()).max().item() / r["y"][..., ok].abs().max().item()
    return first + (2.0 ** -25 if fed else VAR_TOL / 2) + 8 * 2.0 ** -24


def check_out(r, key, got, out_dtype, what, fed=None):
    """an output or gradient against f64: at most 4 x torch f32's error + one rounding of the output dtype, relative to max |ref|;
    y (``fed`` given) is capped by y_cap as well"""
    ok = r["ok"]
    ref = r[key][..., ok]
    got = got.double().cpu()[..., ok]
    scale = ref.abs().max().clamp_min(1e-300).item()
    err = (got - ref).abs().max().item() / scale
    tol = 4 * r["torch_err"][key]
    if key == "y" and fed is not None:
        tol = min(tol, y_cap(r, fed))
    tol += ROUNDING[out_dtype]
    print(f"BNCOND {what} {key}: kernel {err:.3e} torch f32 {r['torch_err'][key]:.3e} bound {tol:.3e}")
    assert torch.isfinite(got).all(), f"{what} {key}: not finite"
    assert err <= tol, f"{what} {key}: error {err:.3e} > {tol:.3e} (torch f32: {r['torch_err'][key]:.3e})"


def dev(r, dtype):
    d = lambda t: t.to(DEV)          # noqa: E731
    return d(r["x"].to(dtype)), d(r["gamma"]), d(r["beta"]), d(r["rm0"].clone()), d(r["rv0"].clone()), d(r["dy"].to(dtype))


def tag(name, shape, rung, std, dtype):
    return f"{name} {'x'.join(map(str, shape))} {'f32' if dtype == torch.float32 else 'bf16'} rung={rung:g} std={std:g}"


# ------------------------------------------------------------------------------------------------ stand-alone producers
@pytest.mark.parametrize("std", SCALES)
@pytest.mark.parametrize("rung", RUNGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", STATS_SHAPES)
def test_bn_stats_ladder(shape, dtype, rung, std):
    r = case(shape, rung, std, dtype)
    assert_reached(r, dtype, "input")
    assert r["torch_var_err"] <= VAR_TOL, "torch's own f32 x.var() misses the bound: the bound is wrong"
    x, g, b, rm, rv, _ = dev(r, dtype)
    mean, var = ops.bn_stats(x, rm, rv, MOM)
    check_stats(r, mean, var, rm, rv, tag("bn_stats", shape, rung, std, dtype))


@pytest.mark.parametrize("rung", [3.0, 5.0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 31, 9, 32), (1, 64, 64, 64)])
def test_bn_stats_either_side_of_the_plain_sum_threshold(shape, dtype, rung):
    """bn_stats keeps the plain sums of x and x^2 up to kappa = 4 and takes the pivoted sums beyond: the same bounds just below and
    just above the switch"""
    r = case(shape, rung, 1.0, dtype)
    assert_reached(r, dtype, "input")
    assert (r["kappa"] < 4.0).all() if rung < 4.0 else (r["kappa"] > 4.0).all()
    x, g, b, rm, rv, _ = dev(r, dtype)
    mean, var = ops.bn_stats(x, rm, rv, MOM)
    check_stats(r, mean, var, rm, rv, tag("bn_stats", shape, rung, 1.0, dtype))


@pytest.mark.parametrize("std", SCALES)
@pytest.mark.parametrize("rung", RUNGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SMALL_SHAPES)
def test_bn_small_fwd_ladder(shape, dtype, rung, std):
    r = case(shape, rung, std, dtype)
    assert_reached(r, dtype, "input")
    x, g, b, rm, rv, _ = dev(r, dtype)
    assert ops.bn_small_fits(x)
    y, mean, var = ops.bn_small_fwd(x, g, b, EPS, False, rm, rv, MOM)
    what = tag("bn_small_fwd", shape, rung, std, dtype)
    check_stats(r, mean, var, rm, rv, what)
    check_out(r, "y", y, dtype, what, fed=False)


# ------------------------------------------------------------------------------------------------ consumers, fed the reference statistics
@pytest.mark.parametrize("act", ["none", "relu", "gelu"])
@pytest.mark.parametrize("std", SCALES)
@pytest.mark.parametrize("rung", RUNGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", STATS_SHAPES)
def test_consumers_fed_reference_statistics(shape, dtype, rung, std, act):
    """(x - mean) rsqrt(var + eps) itself at large |mean|: apply, both backward passes, the one-launch backward and the GELU
    kernels with the f64 statistics rounded to f32."""
    r = case(shape, rung, std, dtype, act=act)
    x, g, b, _, _, dy = dev(r, dtype)
    mean, var = r["mean"].float().to(DEV), r["var"].float().to(DEV)
    what = tag(f"fed/{act}", shape, rung, std, dtype)
    if act == "gelu":
        check_out(r, "y", ops.bn_gelu_apply(x, mean, var, g, b, EPS), dtype, what + " bn_gelu_apply", fed=True)
        dg, db = ops.bn_gelu_bwd_reduce(x, dy, mean, var, g, b, EPS)
        check_out(r, "dg", dg, torch.float32, what + " bn_gelu_bwd_reduce")
        check_out(r, "db", db, torch.float32, what + " bn_gelu_bwd_reduce")
        check_out(r, "dx", ops.bn_gelu_bwd_dx(x, dy, mean, var, g, b, EPS, dg, db, r["P"]), dtype, what + " bn_gelu_bwd_dx")
        return
    relu = act == "relu"
    check_out(r, "y", ops.bn_apply(x, mean, var, g, b, EPS, relu), dtype, what + " bn_apply", fed=True)
    dg, db = ops.bn_bwd_reduce(x, dy, mean, var, g, b, EPS, relu)
    check_out(r, "dg", dg, torch.float32, what + " bn_bwd_reduce")
    check_out(r, "db", db, torch.float32, what + " bn_bwd_reduce")
    check_out(r, "dx", ops.bn_bwd_dx(x, dy, mean, var, g, b, EPS, relu, dg, db, r["P"]), dtype, what + " bn_bwd_dx")
    dx, dg, db = ops.bn_small_bwd(x, dy, mean, var, g, b, EPS, relu)
    check_out(r, "dg", dg, torch.float32, what + " bn_small_bwd")
    check_out(r, "db", db, torch.float32, what + " bn_small_bwd")
    check_out(r, "dx", dx, dtype, what + " bn_small_bwd")


# ------------------------------------------------------------------------------------------------ edges, once per stand-alone producer
def _produce(producer, x, g, b, rm, rv):
    if producer == "bn_stats":
        mean, var = ops.bn_stats(x, rm, rv, MOM)
        return ops.bn_apply(x, mean, var, g, b, EPS, False), mean, var
    return ops.bn_small_fwd(x, g, b, EPS, False, rm, rv, MOM)


PRODUCERS = [("bn_stats", torch.float32), ("bn_stats", torch.bfloat16), ("bn_small_fwd", torch.float32), ("bn_small_fwd", torch.bfloat16)]


@pytest.mark.parametrize("producer,dtype", PRODUCERS)
def test_edge_constant_channel(producer, dtype):
    """a channel that is exactly 1000.125 (bf16 stores 1000): no variance out of round-off, output = beta"""
    shape = (2, 9, 7, 64)
    r = case(shape, 0.25, 1.0, dtype, special="const")
    x, g, b, rm, rv, _ = dev(r, dtype)
    y, mean, var = _produce(producer, x, g, b, rm, rv)
    check_stats(r, mean, var, rm, rv, tag(f"edge/const {producer}", shape, 0.25, 1.0, dtype))
    assert r["var"][2].item() == 0.0
    assert var[2].item() <= VAR_TOL * EPS, var[2].item()
    yc = y[..., 2].double().cpu()
    assert torch.isfinite(yc).all()
    # (x - mean) is at most the mean's bound, 2 ulps of 1000.125, times rsqrt(eps) gamma; plus one rounding of the output
    tol = (2 * 2.0 ** -14 / math.sqrt(EPS) * abs(r["gamma"][2].item())
           + ROUNDING[dtype] * max(abs(r["beta"][2].item()), 1e-3))
    assert (yc - r["beta"][2].double()).abs().max().item() <= tol
    check_out(r, "y", y, dtype, f"edge/const {producer}", fed=False)


@pytest.mark.parametrize("producer,dtype", PRODUCERS)
def test_edge_one_ill_conditioned_channel_among_tame_ones(producer, dtype):
    """kappa = 1000 in one channel of a vectorised 4- / 8-channel lane group must not reach its kappa = 0.25 neighbours"""
    shape = (2, 9, 7, 64)
    r = case(shape, 1000.0, 1.0, dtype, special="mixed")
    assert r["kappa"][5] >= kappa_floor(1000.0, dtype) and (r["kappa"][torch.arange(64) != 5] < 0.3).all()
    x, g, b, rm, rv, _ = dev(r, dtype)
    y, mean, var = _produce(producer, x, g, b, rm, rv)
    what = tag(f"edge/mixed {producer}", shape, 1000.0, 1.0, dtype)
    check_stats(r, mean, var, rm, rv, what)
    check_out(r, "y", y, dtype, what, fed=False)


@pytest.mark.parametrize("pixels", [2, 1])
@pytest.mark.parametrize("producer,dtype", PRODUCERS)
def test_edge_two_pixels_and_one_pixel(producer, dtype, pixels):
    shape = (pixels, 1, 1, 64)
    r = case(shape, 1000.0, 1.0, dtype)
    x, g, b, rm, rv, _ = dev(r, dtype)
    y, mean, var = _produce(producer, x, g, b, rm, rv)
    # one pixel: the unbiased variance does not exist (torch refuses the call): the running variance is not compared
    check_stats(r, mean, var, rm, rv, tag(f"edge/P={pixels} {producer}", shape, 1000.0, 1.0, dtype), running_var=pixels > 1)
    assert torch.isfinite(y.float()).all()
    if pixels == 1:
        assert (var == 0).all() and torch.equal(mean.cpu(), r["x"].reshape(-1))


@pytest.mark.parametrize("rung", RUNGS)
@pytest.mark.parametrize("producer,dtype", PRODUCERS)
def test_edge_negative_mean(producer, dtype, rung):
    shape = (2, 31, 9, 32)
    r = case(shape, rung, 1.0, dtype, sign=-1)
    assert (r["mean"] < 0).all()
    assert_reached(r, dtype, "input")
    x, g, b, rm, rv, _ = dev(r, dtype)
    y, mean, var = _produce(producer, x, g, b, rm, rv)
    what = tag(f"edge/negative {producer}", shape, rung, 1.0, dtype)
    check_stats(r, mean, var, rm, rv, what)
    check_out(r, "y", y, dtype, what, fed=False)


# ------------------------------------------------------------------------------------------------ fused producers
# The GEMM epilogue and the resized-conv forward sums add x and x^2 as they leave the tile: no value of the channel is in hand
# before the tile is done, so there is no pivot, and var = E[x^2] - mean^2 comes from plain f32 partial sums.  Their statistics
# are DEFINED over the bf16-rounded tensor the kernel returned, and that is what keeps them accurate: squares of 8-bit
# significands have 16 bits, and a partial row of 64 .. 128 of them is EXACT in f32 while the values share a binade or two --
# which a large kappa brings about.  The GEMM epilogue (64-row partials) is held to the stand-alone bounds on every rung
# (measured <= 7e-8).  The cell kernel of the resized-conv forward sum adds longer rows and does round when the values straddle
# binades (measured 3e-5 on the kappa = 30 rung; 1.5e-3 at kappa = 258 on another draw of the same shape): it is held to its
# declared range (kappa <= 30 at 1e-4 (v + eps)) and to the 1e-5 bound on the rungs beyond, where a miss
# is a strict expected failure with the measured error in the reason (TAPSUM_XFAIL).
FUSED_VAR_TOL = 1e-4


class OutsideDeclaredRange(AssertionError):
    """the only failure the strict xfail marks below accept: the variance bound missed on a rung beyond the declared range"""


def fused_stats_reference(y, rung, scale):
    C = y.shape[-1]
    y64 = y.float().cpu().double().reshape(-1, C)
    m, v = y64.mean(0), y64.var(0, unbiased=False)
    P = y64.shape[0]
    return dict(P=P, C=C, mean=m, var=v, kappa=m.abs() / v.sqrt().clamp_min(1e-300), rung=rung, std=scale,
                rm=MOM * m, rv=(1 - MOM) + MOM * v * P / (P - 1))


# smallest shapes for which gdl_conv_gemm_stats_rows() is non-zero: B, H, W shrunk from the rows of
# test_conv_gemm_emits_batchnorm_partial_statistics (N = 256: 4 x 72 x 72 emits 324 rows; 2 x 72 x 72 and 4 x 36 x 36 emit none)
GEMM_SHAPES = [(4, 72, 72, 64, 256, 1), (4, 72, 72, 64, 256, 3)]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("rung", RUNGS)
@pytest.mark.parametrize("B,H,W,C,N,R", GEMM_SHAPES)
def test_gemm_epilogue_statistics_ladder(B, H, W, C, N, R, rung, scale):
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(_seed(B, H, W, C, N, R))
    x = torch.randn(B, H, W, C, generator=g).to(DEV, dtype)
    sigma = scale                                                      # std of the output: K products of N(0, 1) x N(0, sigma^2 / K)
    w = (torch.randn(N, R * R * C, generator=g) * (sigma / math.sqrt(R * R * C))).to(DEV, dtype)
    bias = torch.full((N,), rung * sigma).to(DEV)                      # kappa is driven through the bias
    y, partials, rows = ops.conv_gemm(x, w, R=R, S=R, pad=R // 2, bias=bias, want_stats=True)
    assert rows > 0, "this shape no longer emits statistics"
    rm, rv = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
    mean, var = ops.bn_stats_finalize(partials, rows, N, B * H * W, rm, rv, MOM)
    r = fused_stats_reference(y, rung, scale)
    what = f"gemm_epilogue {R}x{R} M={B * H * W} rung={rung:g} std={scale:g}"
    assert_reached(r, dtype, what)
    check_stats(r, mean, var, rm, rv, what)


TAPSUM_CASES = [(2, 16, 24, 64, 2),       # cell kernel
                (1, 4, 16, 64, 4)]        # rolling-window kernel
# Two draws per rung.  "centred": addend = rung x the sum's own spread LESS its own mean, every channel exactly on the rung --
# at kappa >= 300 the bf16 outputs of a channel then share a binade and the sums are exact.  "plain": addend = rung x spread, the
# channels' own means left in, so that channels sit at different places of their binade and some straddle an edge -- the draw
# on which the cell kernel rounds.  (shape, rung, scale, draw) -> measured variance error / (v + eps) of the cases beyond the
# declared range that miss the 1e-5 bound: strict expected failures.
TAPSUM_XFAIL = {((2, 16, 24, 64, 2), 300.0, 1.0, "plain"): 1.5e-3}


def _tapsum_params():
    out = []
    for shape in TAPSUM_CASES:
        for rung in RUNGS:
            for scale in SCALES:
                for draw in ("centred", "plain") if rung > 30.0 else ("centred",):
                    err = TAPSUM_XFAIL.get((shape, rung, scale, draw))
                    marks = () if err is None else pytest.mark.xfail(strict=True, raises=OutsideDeclaredRange, reason=(
                        f"resized-conv forward sum (cell kernel): plain f32 sums of x and x^2, kappa = {rung:g} is outside the declared "
                        f"range (kappa <= 30); measured variance error {err:.1e} (v + eps)"))
                    out.append(pytest.param(*shape, rung, scale, draw, marks=marks))
    return out


@pytest.mark.parametrize("B,H,W,N,f,rung,scale,draw", _tapsum_params())
def test_resized_conv_forward_sum_statistics_ladder(B, H, W, N, f, rung, scale, draw):
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(_seed(B, H, W, N, f))
    z = (torch.randn(B, H // f, W // f, 9 * N, generator=g) * scale).to(DEV, dtype)
    y0 = ops.resize_conv3x3_fwd_sum([z], (H, W)).float().reshape(-1, N)
    # kappa is driven through the per-channel addend (the conv bias)
    add = (rung * y0.std(0, unbiased=False) - y0.mean(0) if draw == "centred" else rung * y0.std(0)).contiguous()
    rm, rv = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
    y, mean, var = ops.resize_conv3x3_fwd_sum_bn([z], (H, W), addvec=add, running_mean=rm, running_var=rv, momentum=MOM)
    r = fused_stats_reference(y, rung, scale)
    what = f"resize_conv3x3_fwd_sum_bn f={f} P={B * H * W} rung={rung:g} std={scale:g} {draw}"
    assert_reached(r, dtype, what)
    if rung > 30.0:      # beyond the declared range only the variance may miss, and only where TAPSUM_XFAIL says so
        ev = ((var.double().cpu() - r["var"]).abs() / (r["var"] + EPS)).max().item()
        if ev > VAR_TOL:
            print(f"BNCOND {what} kappa={r['kappa'].median().item():.4g} var_err={ev:.3e}")
            raise OutsideDeclaredRange(f"{what}: variance off by {ev:.3e} (v + eps)")
    # kappa = 0.25 has nothing to cancel: the stand-alone bound; kappa = 30: the declared one
    check_stats(r, mean, var, rm, rv, what, var_tol=FUSED_VAR_TOL if rung == 30.0 else VAR_TOL)


# ------------------------------------------------------------------------------------------------ SyncBatchNorm merge (no process group)
RANK_PIXELS = (126, 63, 9)


@functools.lru_cache(maxsize=None)
def sync_case(rung, std, C=64, exact_means=True):
    """Three 'ranks' with unequal pixel counts whose means differ by several std; local f64 statistics rounded to f32.
    ``exact_means`` False: the means are rounded as they come, and r["input_term"] is what that rounding alone moves the merged
    variance by: sum_r n_r / n  2 |mean_r - mean| ulp(mean_r) / 2 (the between-rank part (mean_r - mean)^2, first order)."""
    g = torch.Generator().manual_seed(_seed("sync", rung, std))
    shift = (0.0, 3.0, -2.0)
    # (the rank means are up to 5 std apart: the global std is ~1.8 std, so the base mean is 2 kappa std)
    parts = [(torch.randn(n, C, generator=g, dtype=torch.float64) + 2 * rung + s) * std for n, s in zip(RANK_PIXELS, shift)]
    # each rank's mean is made an f32 number (a shift below one f32 ulp): rounding a rank's mean to f32 would otherwise move the
    # between-rank part of the variance by 2 |mean_r - mean| ulp(mean) / 2 -- 2e-5 of it at kappa = 300 -- before any merge runs
    if exact_means:
        parts = [p + (p.mean(0).float().double() - p.mean(0)) for p in parts]
    full = torch.cat(parts)
    m, v = full.mean(0), full.var(0, unbiased=False)
    local = [(p.mean(0).float(), p.var(0, unbiased=False).float(), float(p.shape[0])) for p in parts]
    # the pivot every rank shares (the layer's running_mean): within a few std of the global mean
    pivot = (m + 2.0 * std * torch.randn(C, generator=g, dtype=torch.float64)).float()
    term = sum(p.shape[0] / full.shape[0] * (p.mean(0) - m).abs() * ulp32(p.mean(0)) for p in parts)
    return dict(local=local, mean=m, var=v, kappa=m.abs() / v.sqrt(), pivot=pivot, rung=rung, std=std, P=full.shape[0], C=C,
                input_term=0.0 if exact_means else term)


@pytest.mark.parametrize("exact_means", [True, False])
@pytest.mark.parametrize("path", ["kernels", "torch expressions"])
@pytest.mark.parametrize("std", SCALES)
@pytest.mark.parametrize("rung", RUNGS)
def test_syncbn_merge_ladder(rung, std, path, exact_means):
    """syncbn_pack per rank, a torch add as the all-reduce, syncbn_unpack -- and the torch-expression fallback of
    sync_batch_stats (gnn.sync_message / sync_message_stats) -- against the f64 statistics of the concatenation.  Once with rank
    means that are f32 numbers (the merge arithmetic alone, held to the plain bounds), once with means rounded as they come (what
    bn_stats hands the merge: the bound then carries the input-rounding term, 2e-5 of the variance at kappa = 300)."""
    r = sync_case(rung, std, exact_means=exact_means)
    assert_reached(r, torch.float32, "merged statistics")
    C = r["C"]
    pivot = r["pivot"].to(DEV)
    msgs = []
    for mean, var, n in r["local"]:
        if path == "kernels":
            out = torch.empty(2 * C + 1, device=DEV)
            ops.syncbn_pack(mean.to(DEV), var.to(DEV), n, out, pivot)
        else:
            out = torch.cat(gnn.sync_message(mean.to(DEV), var.to(DEV), n, pivot))
        msgs.append(out)
    packed = msgs[0] + msgs[1] + msgs[2]
    if path == "kernels":
        rm, rv = r["pivot"].clone().to(DEV), torch.ones(C, device=DEV)
        gmean, gvar = ops.syncbn_unpack(packed, C, rm, rv, MOM, pivot=rm)          # the pivot IS the running mean, updated in the same launch
        rm_ref = (1 - MOM) * r["pivot"].double() + MOM * r["mean"]
        assert ((rm.double().cpu() - rm_ref).abs() <= MOM * (2 * ulp32(r["mean"]) + 1e-6 * r["var"].sqrt()) + 2 * ulp32(rm_ref)).all()
    else:
        gmean, gvar, total = gnn.sync_message_stats(packed, C, pivot)
        assert float(total) == float(r["P"])
    check_stats(r, gmean, gvar, None, None, f"syncbn {path} rung={rung:g} std={std:g} {'exact' if exact_means else 'rounded'} rank means",
                input_term=r["input_term"])


def test_syncbn_merge_without_running_buffers():
    """no running buffers: the pivot is 0 (the plain count-weighted message) -- exact to round-off on a tame layer"""
    r = sync_case(0.25, 1.0)
    C = r["C"]
    msgs = []
    for mean, var, n in r["local"]:
        out = torch.empty(2 * C + 1, device=DEV)
        ops.syncbn_pack(mean.to(DEV), var.to(DEV), n, out)
        msgs.append(out)
    gmean, gvar = ops.syncbn_unpack(msgs[0] + msgs[1] + msgs[2], C)
    check_stats(r, gmean, gvar, None, None, "syncbn kernels, no pivot, rung=0.25")
