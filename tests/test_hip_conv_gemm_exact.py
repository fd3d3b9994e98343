"""Exact-integer tests of every forward implicit-GEMM tile (gdl_conv_gemm: csrc/conv_gemm.hip, conv3x3_sf.hip, conv_gemm_dual.hip,
conv3x3_narrow.hip, conv_gemm_w4.hip, conv_gemm_persist.hip, conv_gemm_w4p.hip) and of every epilogue implementation.

Operands are small seeded integers.  They are exact in bf16 and f32, every product is exact, and on the reference side of every
case max|x| * max|w| * R*S*C plus every epilogue term is asserted to stay below 2^24: whatever the summation order in whatever MFMA
accumulator, the f32 result then has exactly one bit pattern.  Every comparison is ``assert_same`` / ``torch.equal`` against a
float64 reference (F.conv2d or a matmul) -- there is no tolerance in this file except the one-rounding bound on the finalized
BatchNorm mean and variance.  A dropped K element, a wrong 16-byte piece of a channel tail, a padding tap read from the
neighbouring row, a tail row taken from the wrong sample, an epilogue constant taken from the neighbouring lane group are hard
failures at any scale.  bf16 outputs: the references are asserted to stay within 2^8, where every integer is a bf16 value.

Every output buffer is allocated here and pre-filled with NaN (channel-slice outputs: with a sentinel on both sides that must
stay bit-unchanged), so an element that is never stored poisons the comparison instead of hiding in the caching allocator.

Every case forces its tile with gdl_debug_force_conv_variant (reset in ``finally``) and asserts through ops.KernelTimer.variants
that gdl_conv_gemm_plan returned this tile for the call (the timer records the plan, which is what gdl_conv_gemm dispatches on, not
the launch itself): a shape for which the hook falls back to the planner's choice fails instead of testing another kernel.  Which
instantiation of tile 5 the plan leads to (tap packed / channel tail / plain) is inferred through the mirror t5_mode.  The
hook checks less than the planner does (the planner only picks 2, 3, 4, 9 and 10 when N % 256 == 0), so every table states the
precondition of the kernel that its shapes rely on.

The tables and the reference helpers are checked without a GPU by tests/test_conv_gemm_exact_host.py.
"""

import contextlib
import functools
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import _lib, ops  # noqa: E402

from test_hip_wgrad_exact import EXACT, assert_same, ints  # noqa: E402

DEV = "cuda"
NAN = float("nan")
BF16_EXACT = 1 << 8                    # every integer of magnitude <= 2^8 is a bf16 value
BF16, F32 = torch.bfloat16, torch.float32
DT_ID = {BF16: "bf16", F32: "f32"}
BKE = {BF16: 64, F32: 32}              # elements of one 128-byte K chunk
# (rows, channels) of one workgroup tile per dispatcher variant (7: 4 x 64 pixels of one image x 32 channels)
TILE = {0: (64, 64), 1: (128, 128), 2: (256, 256), 3: (256, 256), 4: (256, 256), 5: (256, 64), 6: (256, 128), 7: (256, 32),
        8: (256, 256), 9: (256, 256), 10: (256, 256), 12: (64, 64)}
ALL_VARIANTS = tuple(sorted(TILE))

G = namedtuple("G", "B H W C N R S stride pad")


def geo(B, H, W, C, N, R=1, S=None, stride=1, pad=0):
    return G(B, H, W, C, N, R, R if S is None else S, stride, pad)


def out_hw(g):
    return (g.H + 2 * g.pad - g.R) // g.stride + 1, (g.W + 2 * g.pad - g.S) // g.stride + 1


def facts(g, dtype, variant, tap_packed=False):
    """What a table's comment claims about a case: M, workgroup tiles and tails in both dimensions, K-steps."""
    Ho, Wo = out_hw(g)
    M = g.B * Ho * Wo
    bm, bn = TILE[variant]
    kc = -(-g.C // BKE[dtype])
    ksteps = -(-g.R * g.S * g.C // BKE[dtype]) if tap_packed else g.R * g.S * kc
    tiles_m = g.B * (g.H // 4) * (g.W // 64) if variant == 7 else -(-M // bm)
    return dict(M=M, tiles_m=tiles_m, m_tail=M % bm, tiles_n=-(-g.N // bn), n_tail=g.N % bn, ksteps=ksteps)


# ------------------------------------------------------------------ operands, bounds, references
def sparse_ints(shape, seed, keep, dtype=torch.float64):
    """Seeded tensor of -1 / 0 / +1 of which one element in `keep` is non-zero (2 * keep <= 128: the draw is an int8)."""
    assert 1 <= keep <= 64
    gen = torch.Generator().manual_seed(seed)
    r = torch.randint(0, 2 * keep, tuple(shape), generator=gen, dtype=torch.int8)
    return ((r == 1).to(torch.int8) - (r == 0).to(torch.int8)).to(dtype)


def assert_integers(*ts):
    for t in ts:
        if t is not None:
            assert torch.equal(t, t.round()), "operands must be integers"


def assert_exact_bound(x, w, K, e=None):
    """max|x| * max|w| * K, then every epilogue term of `e` in the kernels' order, stays below 2^24: no partial sum of K products
    in any order and no intermediate of the epilogue leaves the integers that f32 holds exactly.  Returns the final bound."""
    e = e or {}
    assert_integers(x, w, *[e.get(k) for k in ("bias", "scale", "shift", "batch_scale", "resid")])
    amax = lambda t: 0.0 if t is None else t.abs().max().item()      # noqa: E731
    m = amax(x) * amax(w) * K
    assert m < EXACT, f"operands are not exact in f32: {m} >= 2^24"
    m += amax(e.get("bias"))
    if e.get("scale") is not None:
        m = m * amax(e["scale"]) + amax(e.get("shift"))
    if e.get("batch_scale") is not None:
        m *= max(amax(e["batch_scale"]), 1.0)
    m += amax(e.get("resid"))
    assert m < EXACT, f"the epilogue leaves the exact integers: {m} >= 2^24"
    return m


def assert_bf16_exact(ref):
    """The reference of a bf16 output: integers within 2^8 are bf16 values, the rounded output is exact too."""
    assert_integers(ref)
    m = ref.abs().max().item()
    assert m <= BF16_EXACT, f"a bf16 output of magnitude {m} > 2^8 is not exact"
    return m


def ref_conv(x, w4, stride, pad):
    """x NHWC [B,H,W,C], w4 [N,C,R,S] (float64) -> NHWC [B,Ho,Wo,N] float64."""
    assert x.dtype == torch.float64 and w4.dtype == torch.float64
    return F.conv2d(x.permute(0, 3, 1, 2), w4, stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


def ref_dgrad(dy, w4, stride, pad, hw):
    """Data gradient of ref_conv: dy NHWC [B,Ho,Wo,N], w4 [N,C,R,S] (float64) -> NHWC [B,H,W,C] float64."""
    assert dy.dtype == torch.float64 and w4.dtype == torch.float64
    x = torch.zeros(dy.shape[0], w4.shape[1], *hw, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w4, stride=stride, padding=pad).backward(dy.permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1).contiguous()


def gemm_weights(w4):
    """[N,C,R,S] -> the kernels' [N, (r, s, c)]."""
    return w4.permute(0, 2, 3, 1).reshape(w4.shape[0], -1).contiguous()


# Per-channel constants: each differs from its neighbours at distance 1, 4, 16 and 64 (7, 5 and 2 are units modulo 19, 17 and 5
# and so are 4, 16 and 64), so a constant fetched from the wrong lane / lane group / 64-channel strip changes the result.
SCALES = (-2.0, -1.0, 1.0, 2.0, 4.0)


def chan_bias(N):
    return ((7 * torch.arange(N)) % 19 - 9).double()


def chan_scale(N):
    return torch.tensor(SCALES, dtype=torch.float64)[(2 * torch.arange(N)) % 5]


def chan_shift(N):
    return ((5 * torch.arange(N)) % 17 - 8).double()


def batch_scales(B):
    return torch.tensor([2.0, 0.0, 1.0], dtype=torch.float64)[torch.arange(B) % 3]


# name -> (scale, shift, activation, batch_scale, resid); every case has the integer bias.  The order of operations is the one
# ops.conv_gemm documents and conv_epilogue implements: x = acc + bias; x = x * scale + shift (shift only with scale); ReLU;
# x *= batch_scale[sample]; x += resid; ReLU again for ACT_RESID_RELU.
EPIS = {
    "bias": (0, 0, "none", 0, 0),
    "bias-relu": (0, 0, "relu", 0, 0),
    "affine-relu": (1, 1, "relu", 0, 0),
    "scale-only": (1, 0, "none", 0, 0),
    "affine-resid": (1, 1, "none", 0, 1),
    "affine-droppath-resid": (1, 1, "none", 1, 1),
    "droppath": (0, 0, "none", 1, 0),
    "resid-relu": (0, 0, "resid_relu", 0, 1),
    "relu-droppath-resid": (0, 0, "relu", 1, 1),
}
ACT = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "resid_relu": ops.ACT_RESID_RELU}


def make_epi(name, B, Ho, Wo, N):
    sc, sh, act, bs, rs = EPIS[name]
    return dict(bias=chan_bias(N), scale=chan_scale(N) if sc else None, shift=chan_shift(N) if sh else None, act=act,
                batch_scale=batch_scales(B) if bs else None, resid=ints((B, Ho, Wo, N), 77 + N, -9, 9) if rs else None)


def ref_epilogue(acc, e):
    """acc NHWC [B,Ho,Wo,N] float64 -> the epilogue's result in float64 (alpha = 1)."""
    x = acc + e["bias"] if e.get("bias") is not None else acc.clone()
    if e.get("scale") is not None:
        x = x * e["scale"] + (e["shift"] if e.get("shift") is not None else 0.0)
    if e.get("act") == "relu":
        x = x.clamp_min(0.0)
    if e.get("batch_scale") is not None:
        x = x * e["batch_scale"].view(-1, 1, 1, 1)
    if e.get("resid") is not None:
        x = x + e["resid"]
    if e.get("act") == "resid_relu":
        x = x.clamp_min(0.0)
    return x


@functools.lru_cache(maxsize=24)
def problem(g, wide):
    """(x NHWC, w4 [N,C,R,S], acc NHWC) in float64 of one geometry, computed once and shared by every tile's case.  wide: x and w
    in -2..2 (f32 outputs); else w in -1..1 and x in -1 / 0 / +1, sparse: eight non-zero activations per output (one in eight for
    K <= 64), so that a bf16 output stays within 2^8 through scale 4, DropPath scale 2 and the residual."""
    seed = 1009 * g.R + 31 * g.C + 7 * g.N + g.H * g.W + g.stride
    if wide:
        x, w4 = ints((g.B, g.H, g.W, g.C), seed), ints((g.N, g.C, g.R, g.S), seed + 1)
    else:
        keep = min(max(8, g.R * g.S * g.C // 8), 64)
        x, w4 = sparse_ints((g.B, g.H, g.W, g.C), seed, keep), ints((g.N, g.C, g.R, g.S), seed + 1, -1, 1)
    assert_exact_bound(x, w4, g.R * g.S * g.C)
    return x, w4, ref_conv(x, w4, g.stride, g.pad)


@functools.lru_cache(maxsize=24)
def device_operands(g, wide, dtype):
    x, w4, _ = problem(g, wide)
    return x.to(DEV, dtype), gemm_weights(w4).to(DEV, dtype)


def big_problem(g, keep, device=None):
    """Operands and accumulator of a dense 1x1 problem too large for a float64 reference on the CPU: x (-1 / 0 / +1, one element in
    `keep` non-zero) and w (-1..1) as f32 tensors, acc [M, N] f32.  The bound makes an f32 matmul of these integers exact; with a
    device the accumulator is torch's own float64 matmul there (rocBLAS, no kernel of this project), in row chunks."""
    assert g.R == 1 and g.S == 1 and g.stride == 1 and g.pad == 0
    M = g.B * g.H * g.W
    x = sparse_ints((M, g.C), 5 + g.C, keep, torch.float32)
    w = ints((g.N, g.C), 6 + g.C, -1, 1).float()
    assert_exact_bound(x, w, g.C)
    parts = []
    for r0 in range(0, M, 16384):
        if device is None:
            parts.append(x[r0:r0 + 16384] @ w.t())
        else:
            parts.append((x[r0:r0 + 16384].to(device).double() @ w.to(device).double().t()).float().cpu())
    return x, w, torch.cat(parts)


# ------------------------------------------------------------------ hooks, output buffers, launcher
HOOKS = {"korder": ("gdl_debug_set_conv_korder", 1), "epilogue": ("gdl_debug_set_conv_epilogue", 1),
         "tap_packing": ("gdl_debug_set_conv_tap_packing", 1), "w4p": ("gdl_debug_set_conv_w4p", 0),
         "ngroup_kb": ("gdl_debug_set_conv_ngroup_kb", 2560), "persist": ("gdl_debug_set_conv_persist", 1),
         "sf": ("gdl_debug_set_conv_sf", 1)}


@contextlib.contextmanager
def forced(variant, **hooks):
    """Force a tile variant (-1: the planner's choice) and set the named gdl_debug_* hooks; yields the KernelTimer whose
    `variants` lists the tile of every launch.  Everything is reset on the way out."""
    lib = _lib.load()
    ops.TIMER = timer = ops.KernelTimer()
    try:
        for k, v in hooks.items():
            getattr(lib, HOOKS[k][0])(int(v))
        lib.gdl_debug_force_conv_variant(int(variant))
        yield timer
    finally:
        lib.gdl_debug_force_conv_variant(-1)
        for k in hooks:
            getattr(lib, HOOKS[k][0])(HOOKS[k][1])
        ops.TIMER = None


GUARD = {"dense": 0, "slice8": 8, "slice3": 3}    # channels on each side of a sliced output: 8 keeps 16-byte alignment, 3 does not
LEFT, RIGHT = 5.0, -7.0


def make_out(B, Ho, Wo, N, dtype, kind):
    """NaN-filled output (a channel slice of a wider buffer with a sentinel on both sides for the slice kinds) -> (buffer, view)."""
    gd = GUARD[kind]
    buf = torch.full((B, Ho, Wo, N + 2 * gd), NAN, device=DEV, dtype=dtype)
    if gd:
        buf[..., :gd], buf[..., gd + N:] = LEFT, RIGHT
    return buf, buf[..., gd:gd + N] if gd else buf


def check_out(buf, view, ref, kind, what):
    if view.dtype == BF16:
        assert_bf16_exact(ref)
    assert_same(view.float(), ref.float(), what)
    gd = GUARD[kind]
    if gd:
        assert torch.equal(buf[..., :gd], torch.full_like(buf[..., :gd], LEFT)), f"{what}: left sentinel written"
        assert torch.equal(buf[..., -gd:], torch.full_like(buf[..., -gd:], RIGHT)), f"{what}: right sentinel written"


def epi_device(e, resid_dtype):
    f = lambda t: None if t is None else t.float().to(DEV)      # noqa: E731
    return dict(bias=f(e.get("bias")), scale=f(e.get("scale")), shift=f(e.get("shift")), act=ACT[e.get("act", "none")],
                batch_scale=f(e.get("batch_scale")), resid=None if e.get("resid") is None else e["resid"].to(DEV, resid_dtype))


def run(variant, dtype, g, *, wide, e=None, out_dtype=F32, kind="dense", resid_dtype=None, what="", **hooks):
    """One forced launch of ops.conv_gemm on a poisoned output, compared bit for bit with the float64 reference."""
    x, w4, acc = problem(g, wide)
    e = e or {}
    assert_exact_bound(x, w4, g.R * g.S * g.C, e)
    ref = ref_epilogue(acc, e)
    xd, wd = device_operands(g, wide, dtype)
    buf, view = make_out(*acc.shape, out_dtype, kind)
    with forced(variant, **hooks) as timer:
        ops.conv_gemm(xd, wd, R=g.R, S=g.S, stride=g.stride, pad=g.pad, out=view, **epi_device(e, resid_dtype or out_dtype))
        torch.cuda.synchronize()
    what = f"variant {variant} {DT_ID[dtype]} {tuple(g)} -> {DT_ID[out_dtype]} {kind} {what} {hooks or ''}"
    assert timer.variants == [variant], f"{what}: the hook fell back to tile {timer.variants}"
    check_out(buf, view, ref, kind, what)


# ------------------------------------------------------------------ 1. the 256^2 tiles: 2, 3 (ping-pong), 8 (one wave per SIMD)
# Preconditions relied on: C a whole number of K chunks (the 256^2 kernels zero-fill no channel tail; the forced branch checks
# it), N % 256 == 0 (what the planner requires; the kernels' N tail is not under test here), for 8 bf16 operands
# (conv_gemm_w4_applicable).  `chunks` = C in 128-byte K chunks, so the K-step count is the same in bf16 and f32.
# (id, B, H, W, chunks, N, R, stride, pad, expected facts).  M = 549 = 2 * 256 + 37; with B = 3 a tile spans the sample boundaries
# at rows 183 and 366.
T256 = [
    ("1x1-kt1", 3, 3, 61, 1, 256, 1, 1, 0, dict(M=549, tiles_m=3, m_tail=37, tiles_n=1, ksteps=1)),
    ("1x1-kt2", 3, 3, 61, 2, 512, 1, 1, 0, dict(M=549, tiles_m=3, m_tail=37, tiles_n=2, ksteps=2)),
    ("1x1-kt3", 3, 3, 61, 3, 256, 1, 1, 0, dict(M=549, tiles_m=3, m_tail=37, tiles_n=1, ksteps=3)),
    ("1x1-kt5", 3, 3, 61, 5, 512, 1, 1, 0, dict(M=549, tiles_m=3, m_tail=37, tiles_n=2, ksteps=5)),
    ("3x3-pad1", 2, 9, 17, 1, 256, 3, 1, 1, dict(M=306, tiles_m=2, m_tail=50, tiles_n=1, ksteps=9)),      # sample boundary at row 153
    ("3x3-stride2", 2, 19, 27, 1, 256, 3, 2, 1, dict(M=280, tiles_m=2, m_tail=24, tiles_n=1, ksteps=9)),  # 10 x 14 outputs per sample
    ("8x8-stride8-stem", 1, 136, 136, 1, 256, 8, 8, 0, dict(M=289, tiles_m=2, m_tail=33, tiles_n=1, ksteps=64)),
]


def t256_geo(row, dtype):
    _, B, H, W, chunks, N, R, stride, pad, _ = row
    return geo(B, H, W, chunks * BKE[dtype], N, R, stride=stride, pad=pad)


@pytest.mark.parametrize("row", T256, ids=[r[0] for r in T256])
@pytest.mark.parametrize("variant,dtype", [(2, BF16), (2, F32), (3, BF16), (3, F32), (8, BF16)],
                         ids=["v2-bf16", "v2-f32", "v3-bf16", "v3-f32", "v8-bf16"])
def test_tiles_256(variant, dtype, row):
    """1x1 dense with an M tail, 3x3 pad 1, 3x3 stride 2 and an 8x8 / stride-8 patch stem at N = 256 and 512; 1, 2, 3 and 5
    K-steps for the ping-pong parity (2, 3) and for the separate last-two-steps instantiations (8)."""
    g = t256_geo(row, dtype)
    assert {k: facts(g, dtype, variant)[k] for k in row[-1]} == row[-1]
    run(variant, dtype, g, wide=True, e=dict(bias=chan_bias(g.N)))


def test_tile_w4_data_gradient():
    """Variant 8 on the data gradient of a 3x3 / pad 1 convolution (256 -> 64 channels) through ops.pack_dgrad: the flipped,
    transposed filter with pad = R - 1 - pad.  As a GEMM: C = 64 (9 K-steps), N = 256, M = 306."""
    B, H, W, Cin, Nout = 2, 9, 17, 256, 64
    w4, dy = ints((Nout, Cin, 3, 3), 91), ints((B, H, W, Nout), 92)
    assert_exact_bound(dy, w4, 9 * Nout)
    ref = ref_dgrad(dy, w4, 1, 1, (H, W))
    wd = ops.pack_dgrad(gemm_weights(w4).float().to(DEV), Nout, 9, Cin, BF16)
    buf, view = make_out(B, H, W, Cin, F32, "dense")
    with forced(8) as timer:
        ops.conv_gemm(dy.to(DEV, BF16), wd, R=3, S=3, pad=3 - 1 - 1, out=view)
        torch.cuda.synchronize()
    assert timer.variants == [8]
    check_out(buf, view, ref, "dense", "variant 8, data gradient of a 3x3")


# ------------------------------------------------------------------ 2. tile 4: 3x3 with shared activation staging
# Preconditions relied on (conv3x3_sf_applicable): 3x3 / stride 1 / pad 1, pixel-dense input, nz = 1, N % 256 == 0; C a whole
# number of K chunks in both dtypes.  The kernel stages 288 pixels of the flattened NHWC stream per (chunk, filter row): W = 5 is
# shorter than, 16 divides and 23 does not divide that length; with H = 1 and 2 every output row is a border row; B = 3 puts the
# sample boundaries inside the one 256-row tile (the last case has two tiles and an M tail).
# (id, B, H, W, C, expected facts; ksteps as (bf16, f32))
TSF = [
    ("h1-w5-c64", 3, 1, 5, 64, dict(M=15, tiles_m=1, m_tail=15), (9, 18)),
    ("h2-w16-c192", 3, 2, 16, 192, dict(M=96, tiles_m=1, m_tail=96), (27, 54)),
    ("h2-w23-c64", 3, 2, 23, 64, dict(M=138, tiles_m=1, m_tail=138), (9, 18)),
    ("h1-w23-c192", 3, 1, 23, 192, dict(M=69, tiles_m=1, m_tail=69), (27, 54)),
    ("h7-w16-c64", 3, 7, 16, 64, dict(M=336, tiles_m=2, m_tail=80), (9, 18)),
]


@pytest.mark.parametrize("row", TSF, ids=[r[0] for r in TSF])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_tile_shared_staging(dtype, row):
    _, B, H, W, Cc, want, ksteps = row
    g = geo(B, H, W, Cc, 256, 3, pad=1)
    f = facts(g, dtype, 4)
    assert {k: f[k] for k in want} == want and f["ksteps"] == ksteps[dtype == F32]
    run(4, dtype, g, wide=True, e=dict(bias=chan_bias(256)))


# ------------------------------------------------------------------ 3. tile 5: 256 x 64, plain / channel tail / tap packed
# Preconditions relied on: N <= 64 (the forced branch checks it), C a multiple of 16 bytes (gdl_conv_gemm checks it); tap
# packing needs C < one K chunk and a divisor of it, R*S <= 32 and a filter that is not 1x1 (gdl_conv_gemm's `tap_packed`).
# M = 286 = 256 + 30 in every case: 3x3 / pad 1 on 2 x 11 x 13, 2x2 / stride 2 on 2 x 22 x 26.
# (id, dtype, C, filter, mode, K-steps with tap packing, K-steps without)
T5 = [
    ("bf16-plain-c64", BF16, 64, "3x3", "plain", 9, 9), ("f32-plain-c32", F32, 32, "3x3", "plain", 9, 9),
    ("bf16-ctail-c72", BF16, 72, "3x3", "ctail", 18, 18), ("bf16-ctail-c40", BF16, 40, "3x3", "ctail", 9, 9),
    ("f32-ctail-c36", F32, 36, "3x3", "ctail", 18, 18),
    ("bf16-tap-c8-3x3", BF16, 8, "3x3", "tap", 2, 9), ("bf16-tap-c16-3x3", BF16, 16, "3x3", "tap", 3, 9),
    ("bf16-tap-c32-3x3", BF16, 32, "3x3", "tap", 5, 9), ("bf16-tap-c8-2x2s2", BF16, 8, "2x2s2", "tap", 1, 4),
    ("bf16-tap-c16-2x2s2", BF16, 16, "2x2s2", "tap", 1, 4), ("bf16-tap-c32-2x2s2", BF16, 32, "2x2s2", "tap", 2, 4),
    ("f32-tap-c4-3x3", F32, 4, "3x3", "tap", 2, 9), ("f32-tap-c8-3x3", F32, 8, "3x3", "tap", 3, 9),
    ("f32-tap-c16-3x3", F32, 16, "3x3", "tap", 5, 9), ("f32-tap-c4-2x2s2", F32, 4, "2x2s2", "tap", 1, 4),
    ("f32-tap-c8-2x2s2", F32, 8, "2x2s2", "tap", 1, 4), ("f32-tap-c16-2x2s2", F32, 16, "2x2s2", "tap", 2, 4),
]
T5_N = (64, 40, 5)                      # a whole tile, a tail of 16-byte pieces, a tail inside one piece


def t5_geo(row, N):
    _, _, Cc, filt, _, _, _ = row
    return geo(2, 11, 13, Cc, N, 3, pad=1) if filt == "3x3" else geo(2, 22, 26, Cc, N, 2, stride=2)


def t5_mode(g, dtype, packing):
    """The instantiation gdl_conv_gemm picks for variant 5 (its `tap_packed` and c_tail)."""
    bke, al = BKE[dtype], BKE[dtype] // 8
    if packing and g.R * g.S > 1 and g.R * g.S <= 32 and g.C < bke and bke % g.C == 0 and g.C >= al:
        return "tap"
    return "ctail" if g.C % bke else "plain"


T5_RUNS = [(r, 1) for r in T5] + [(r, 0) for r in T5 if r[4] == "tap"]


@pytest.mark.parametrize("row,packing", T5_RUNS, ids=[r[0] + ("" if p else "-packing-off") for r, p in T5_RUNS])
def test_tile_narrow_output(row, packing):
    """All three instantiations at N = 64, 40 and 5 with an M tail; the tap-packed shapes run again with
    gdl_debug_set_conv_tap_packing(0), where the channel-tail instantiation takes them."""
    _, dtype, Cc, filt, mode, kt_packed, kt_plain = row
    for N in T5_N:
        g = t5_geo(row, N)
        assert t5_mode(g, dtype, packing) == (mode if packing else "ctail")
        f = facts(g, dtype, 5, tap_packed=bool(packing) and mode == "tap")
        assert (f["M"], f["tiles_m"], f["m_tail"], f["tiles_n"]) == (286, 2, 30, 1)
        assert f["ksteps"] == (kt_packed if packing else kt_plain)
        run(5, dtype, g, wide=True, e=dict(bias=chan_bias(N)), tap_packing=packing)


# ------------------------------------------------------------------ 4. tile 6: dual-resident 256 x 128
# Preconditions relied on (conv_gemm_dual_applicable): bf16, C % 64 == 0.  N = 200 leaves a 72-channel N tail in the second tile
# (and N % 16 != 0: the register epilogue with scalar stores).
T6 = [
    ("1x1-dense", geo(3, 3, 61, 128, 200), dict(M=549, tiles_m=3, m_tail=37, tiles_n=2, n_tail=72, ksteps=2)),
    ("3x3-stride2", geo(2, 19, 27, 64, 200, 3, stride=2, pad=1), dict(M=280, tiles_m=2, m_tail=24, tiles_n=2, n_tail=72, ksteps=9)),
]


@pytest.mark.parametrize("name,g,want", T6, ids=[r[0] for r in T6])
def test_tile_dual_resident(name, g, want):
    assert facts(g, BF16, 6) == want
    run(6, BF16, g, wide=True, e=dict(bias=chan_bias(g.N)))


# ------------------------------------------------------------------ 5. tile 7: direct narrow 3x3
# Preconditions relied on (conv3x3_narrow_applicable): bf16, 3x3 / stride 1 / pad 1, C in {8, 16, 32}, dense NHWC input,
# H % 4 == 0 and W % 64 == 0 (a block owns 4 x 64 pixels), weight rows 16-byte aligned.  N = 32 is one whole 32-channel slice,
# 5 one short slice, 40 a whole and a short one.
T7_HW = {"one-tile": (4, 64), "2x2-tiles": (8, 128)}
T7_N = (32, 5, 40)


@pytest.mark.parametrize("hw", list(T7_HW))
@pytest.mark.parametrize("Cc", [8, 16, 32])
def test_tile_direct_narrow(Cc, hw):
    H, W = T7_HW[hw]
    for N in T7_N:
        g = geo(2, H, W, Cc, N, 3, pad=1)
        f = facts(g, BF16, 7)
        assert (f["tiles_m"], f["tiles_n"], f["n_tail"]) == (2 * (H // 4) * (W // 64), -(-N // 32), N % 32)
        run(7, BF16, g, wide=True, e=dict(bias=chan_bias(N)))


# ------------------------------------------------------------------ 6. tiles 9 and 10: persistent workgroups
def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


# Preconditions relied on (conv_gemm_persist_applicable): bf16, dense 1x1, C % 64 == 0, N % 256 == 0, nz = 1.
MI355X_CUS = 256                        # what the tables are sized for; the GPU tests read the device's own count
G9 = geo(3, 1, 25587, 64, 512)          # M = 76761 = 299 * 256 + 217: 300 x 2 = 600 tiles (88 workgroups of 256 take a third)
# Preconditions relied on (w4p_kind): bf16 in and out, dense 1x1, C % 256 == 0 and C >= 768 (so at least 12 K-steps), N % 256 == 0,
# no residual / DropPath scale, 16-byte aligned pixel-dense output; kind 1 = bias only, kind 2 = scale (+ shift) + ReLU.
G10 = {12: geo(7, 1, 21917, 768, 256), 16: geo(7, 1, 21917, 1024, 256)}   # M = 153419 = 599 * 256 + 75: 600 tiles
PERSISTENT = [(9, G9, dict(M=76761, tiles_m=300, m_tail=217, tiles_n=2, n_tail=0, ksteps=1)),
              (10, G10[12], dict(M=153419, tiles_m=600, m_tail=75, tiles_n=1, n_tail=0, ksteps=12)),
              (10, G10[16], dict(M=153419, tiles_m=600, m_tail=75, tiles_n=1, n_tail=0, ksteps=16))]
BIG_KEEP = {9: 4, 10: 16}                # one activation in 4 (K = 64) / 16 (K >= 768) is non-zero: the bf16 outputs stay within 2^8


def run_big(variant, g, cases, **hooks):
    """`cases`: (name, epilogue, output kind).  Operands are uploaded once; the accumulator is torch's float64 matmul on the
    device (see big_problem)."""
    f = facts(g, BF16, variant)
    tiles = f["tiles_m"] * f["tiles_n"]
    assert tiles > 2 * cu_count(), f"{tiles} tiles do not give every workgroup of {cu_count()} CUs a second and a third tile"
    assert f["m_tail"] != 0
    x, w, acc = big_problem(g, BIG_KEEP[variant], DEV)
    acc = acc.double().view(g.B, g.H, g.W, g.N)
    xd, wd = x.to(DEV).to(BF16).view(g.B, g.H, g.W, g.C), w.to(DEV, BF16)
    for name, e, kind in cases:
        assert_exact_bound(x, w, g.C, e)
        ref = ref_epilogue(acc, e)
        buf, view = make_out(g.B, g.H, g.W, g.N, BF16, kind)
        with forced(variant, **hooks) as timer:
            ops.conv_gemm(xd, wd, out=view, **epi_device(e, BF16))
            torch.cuda.synchronize()
        assert timer.variants == [variant], f"{name}: the hook fell back to tile {timer.variants}"
        check_out(buf, view, ref, kind, f"variant {variant} {tuple(g)} {name} {kind}")


def test_tile_persistent():
    """Variant 9 with more than two tiles per CU (workgroups take a second and a third tile), one K-step, an M tail."""
    assert facts(G9, BF16, 9) == PERSISTENT[0][2]
    N = G9.N
    run_big(9, G9, [("bias", dict(bias=chan_bias(N)), "dense"),
                    ("affine-relu", dict(bias=chan_bias(N), scale=chan_scale(N), shift=chan_shift(N), act="relu"), "slice8")])


@pytest.mark.parametrize("ksteps", [12, 16])
def test_tile_parked(ksteps):
    """Variant 10: the `KT == 12` and the `more` instantiations, kinds 1 (plain) and 2 (scale + ReLU) of w4p_kind, the rows past
    M dropped by the store descriptor, dense and into an aligned channel slice.  (The tile is opt-in: gdl_debug_set_conv_w4p(1).)"""
    g = G10[ksteps]
    assert facts(g, BF16, 10) == [p[2] for p in PERSISTENT if p[1] == g][0]
    N = g.N
    affine = dict(bias=chan_bias(N), scale=chan_scale(N), shift=chan_shift(N), act="relu")
    run_big(10, g, [("kind1", dict(bias=chan_bias(N)), "dense"), ("kind1", dict(bias=chan_bias(N)), "slice8"),
                    ("kind2", affine, "dense"), ("kind2-noshift", dict(affine, shift=None), "slice8")], w4p=1)


# ------------------------------------------------------------------ 7. tile 12: 64^2 with four LDS stages
# Preconditions relied on: bf16, C % 64 == 0 (the forced branch checks both).  The prologue issues `if (t < KT)` tiles 0..3 and
# waits for min(KT - 1, 3) younger tiles, the loop's wait counts `last - (kt + 1)` with last clamped to KT - 1: every KT >= 1
# is supported, so the smallest is 1 and nothing needs to fall back.  KT = 1, stages - 1, stages, stages + 1, and a long K.
# M = 165 = 2 * 64 + 37, N = 72 = 64 + 8 (N % 16 != 0: scalar stores).
T12 = [("kt1", geo(3, 5, 11, 64, 72), 1), ("kt3", geo(3, 5, 11, 192, 72), 3), ("kt4", geo(3, 5, 11, 256, 72), 4),
       ("kt5", geo(3, 5, 11, 320, 72), 5), ("kt27-3x3", geo(3, 5, 11, 192, 72, 3, pad=1), 27), ("kt17", geo(3, 5, 11, 1088, 72), 17)]


@pytest.mark.parametrize("name,g,ksteps", T12, ids=[r[0] for r in T12])
def test_tile_four_stages(name, g, ksteps):
    assert facts(g, BF16, 12) == dict(M=165, tiles_m=3, m_tail=37, tiles_n=2, n_tail=8, ksteps=ksteps)
    run(12, BF16, g, wide=True, e=dict(bias=chan_bias(g.N)))


def test_four_stage_hook_falls_back_for_f32():
    """The forced branch's own check: f32 operands do not reach the four-stage tile (it has no f32 instantiation)."""
    g = geo(3, 5, 11, 64, 72)
    x, w4, acc = problem(g, True)
    buf, view = make_out(*acc.shape, F32, "dense")
    with forced(12) as timer:
        ops.conv_gemm(*device_operands(g, True, F32), out=view)
        torch.cuda.synchronize()
    assert timer.variants == [0], timer.variants
    check_out(buf, view, acc, "dense", "forced 12 on f32 operands")


# ------------------------------------------------------------------ 8. tiles 0 and 1: batched call, aux_out
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_small_tiles_batched_conv_transpose_phases(dtype, variant):
    """One batched call, nz = 4, nz_inner = 2, laid out as ops.convt2x2 lays out the four output phases of a ConvTranspose2d(k 2,
    s 2): z = (row phase, column phase) selects the filter through w_sZ and the strided output positions through out_sZ."""
    B, H, W, cin, cout = 2, 5, 7, 24, 40
    x, w = ints((B, H, W, cin), 41), ints((cin, cout, 2, 2), 42)
    bias = chan_bias(cout)
    assert_exact_bound(x, w, cin, dict(bias=bias))
    ref = F.conv_transpose2d(x.permute(0, 3, 1, 2), w, bias, stride=2).permute(0, 2, 3, 1).contiguous()
    xd, wf = x.to(DEV, dtype), w.permute(2, 3, 1, 0).contiguous().to(DEV, dtype)       # [py, px, Cout, Cin]
    bd = bias.float().to(DEV)
    y = torch.full((B, 2 * H, 2 * W, cout), NAN, device=DEV, dtype=F32)
    a = ops.ConvArgs()
    a.inp, a.dtype = xd.data_ptr(), ops.dt(xd)
    a.B, a.H, a.W, a.C = B, H, W, cin
    a.in_sB, a.in_sH, a.in_sW = xd.stride(0), xd.stride(1), xd.stride(2)
    a.Ho, a.Wo, a.R, a.S, a.stride, a.pad = H, W, 1, 1, 1, 0
    a.w, a.w_sN, a.N = wf.data_ptr(), cin, cout
    a.out, a.out_dtype = y.data_ptr(), ops.dt(y)
    a.out_sB, a.out_sH, a.out_sW = y.stride(0), 2 * y.stride(1), 2 * y.stride(2)
    a.alpha, a.act, a.bias = 1.0, ops.ACT_NONE, bd.data_ptr()
    a.nz, a.nz_inner = 4, 2
    a.w_sZ0, a.w_sZ1 = 2 * cout * cin, cout * cin
    a.out_sZ0, a.out_sZ1 = y.stride(1), y.stride(2)
    with forced(variant) as timer:
        ops.batched_gemm_raw(a)
        torch.cuda.synchronize()
    assert timer.variants == [variant]
    assert_same(y, ref.float(), f"variant {variant} {DT_ID[dtype]}: four ConvTranspose phases in one batched call")


AUX_OUT = [("dense", F32), ("dense", BF16), ("slice3", F32), ("slice3", BF16)]


@pytest.mark.parametrize("kind,out_dtype", AUX_OUT, ids=[f"{k}-{DT_ID[d]}" for k, d in AUX_OUT])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_small_tiles_aux_out(dtype, variant, kind, out_dtype):
    """`aux_out` receives acc + bias, `out` the ReLU of the affine map of it -- through the coalesced row epilogue (dense,
    tile 1), the register epilogue (tile 0) and its scalar stores (unaligned slice)."""
    g = geo(3, 13, 21, 64, 128)
    wide = out_dtype == F32
    x, w4, acc = problem(g, wide)
    e = dict(bias=chan_bias(g.N), scale=chan_scale(g.N), shift=chan_shift(g.N), act="relu")
    assert_exact_bound(x, w4, g.C, e)
    xd, wd = device_operands(g, wide, dtype)
    buf, view = make_out(*acc.shape, out_dtype, kind)
    abuf, aview = make_out(*acc.shape, out_dtype, kind)
    with forced(variant) as timer:
        ops.conv_gemm(xd, wd, out=view, aux_out=aview, **epi_device(e, out_dtype))
        torch.cuda.synchronize()
    assert timer.variants == [variant]
    check_out(buf, view, ref_epilogue(acc, e), kind, f"variant {variant} out")
    check_out(abuf, aview, acc + e["bias"], kind, f"variant {variant} aux_out")


# ------------------------------------------------------------------ 9. the epilogue, on every implementation
# conv_epilogue_rows2 (the coalesced row epilogue; its compile-time and, with the hook at 2, its run-time form), conv_epilogue_rows
# (the hook at 0; also what residuals of the other dtype and M-tail waves take), the register epilogue (tiles 0, 12 and 7, every
# unaligned or N % 16 != 0 output), and the tiles in conv_gemm_w4.hip / conv_gemm_dual.hip / conv3x3_sf.hip / conv_gemm_persist.hip
# that call them with their own wave geometry.  (conv_gemm_w4p.hip's phase 1 takes only kinds 1 and 2: test_tile_parked.)
# HoWo = 273 >= 256 lets a DropPath scale through the coalesced epilogue, and the sample boundaries (rows 273, 546 of M = 819 =
# 3 * 256 + 51) fall inside 32-row passes; tile 7 needs W % 64 == 0: HoWo = 256.
EPI_GEO = {0: geo(3, 13, 21, 64, 128), 1: geo(3, 13, 21, 64, 128), 2: geo(3, 13, 21, 64, 256), 3: geo(3, 13, 21, 64, 256),
           4: geo(3, 13, 21, 64, 256, 3, pad=1), 5: geo(3, 13, 21, 64, 64), 6: geo(3, 13, 21, 64, 256),
           7: geo(3, 4, 64, 16, 64, 3, pad=1), 8: geo(3, 13, 21, 64, 256), 9: geo(3, 13, 21, 64, 256), 12: geo(3, 13, 21, 64, 128)}
EPI_TILES = [(0, BF16), (0, F32), (1, BF16), (1, F32), (2, BF16), (2, F32), (3, BF16), (3, F32), (4, BF16), (4, F32), (5, BF16), (5, F32),
             (6, BF16), (7, BF16), (8, BF16), (9, BF16), (12, BF16)]
COALESCED = (1, 2, 3, 4, 5, 6, 8, 9)    # tiles whose waves own 64 channels and hand conv_epilogue an LDS buffer


def epi_geo(variant, dtype):
    g = EPI_GEO[variant]
    return g._replace(C=g.C // 2) if dtype == F32 and variant != 7 else g      # one K chunk in either dtype


@pytest.mark.parametrize("name", list(EPIS))
@pytest.mark.parametrize("variant,dtype", EPI_TILES, ids=[f"v{v}-{DT_ID[d]}" for v, d in EPI_TILES])
def test_epilogue(variant, dtype, name):
    """Integer bias, scale in {-2, -1, 1, 2, 4}, integer shift, DropPath scale in {0, 1, 2}, integer residual in f32 and bf16,
    ReLU before and after the residual -- into f32 and bf16, dense and into aligned / unaligned channel slices."""
    g = epi_geo(variant, dtype)
    Ho, Wo = out_hw(g)
    e = make_epi(name, g.B, Ho, Wo, g.N)
    resid_dtypes = (F32, BF16) if e["resid"] is not None else (None,)
    for out_dtype in (F32, BF16):
        for rdt in resid_dtypes:
            for kind in GUARD:
                run(variant, dtype, g, wide=out_dtype == F32, e=e, out_dtype=out_dtype, kind=kind, resid_dtype=rdt,
                    what=f"{name} resid {rdt}")
            if variant in COALESCED:
                for setting in (0, 2):
                    run(variant, dtype, g, wide=out_dtype == F32, e=e, out_dtype=out_dtype, resid_dtype=rdt,
                        what=f"{name} resid {rdt}", epilogue=setting)


# ------------------------------------------------------------------ 10. K order
# One 3x3 / pad 1 case with two channel chunks per tap (C = 128 bf16 / 64 f32) per tile family, under both values of
# gdl_debug_set_conv_korder.  (4, 6 and 8 have one K order of their own; the hook must not disturb them.)
KORDER_TILES = [(0, BF16), (0, F32), (1, BF16), (1, F32), (2, BF16), (2, F32), (3, BF16), (3, F32), (4, BF16), (4, F32), (5, BF16), (5, F32), (6, BF16),
                (8, BF16), (12, BF16)]


@pytest.mark.parametrize("tap_inner", [1, 0], ids=["tap-inner", "tap-outer"])
@pytest.mark.parametrize("variant,dtype", KORDER_TILES, ids=[f"v{v}-{DT_ID[d]}" for v, d in KORDER_TILES])
def test_k_order(variant, dtype, tap_inner):
    g = geo(2, 9, 17, 2 * BKE[dtype], 64 if variant == 5 else 256, 3, pad=1)
    assert facts(g, dtype, variant)["ksteps"] == 18
    run(variant, dtype, g, wide=True, e=dict(bias=chan_bias(g.N)), korder=tap_inner)


# ------------------------------------------------------------------ 11. N grouping of the tile order
def conv_n_group(R, S, Cc, es, N, bm, bn, conc, budget_kb):
    """Python mirror of conv_n_group (csrc/conv_gemm.hip): N tiles per group for bm x bn tiles of which an XCD runs `conc` at a
    time, with `budget_kb` KiB of L2 for one group's weight panels; 0 = no grouping."""
    budget = budget_kb * 1024
    if budget <= 0:
        return 0
    kbytes = R * S * Cc * es
    a_panel, w_panel = bm * kbytes, bn * kbytes
    tiles_n = -(-N // bn)
    w_fit = budget // w_panel
    if w_fit < 1 or w_fit >= tiles_n:
        return 0

    def cost(w):
        wc = min(w, conc)
        return (conc // wc) * a_panel + (0 if w * w_panel <= budget else wc * w_panel)

    if cost(w_fit) >= cost(tiles_n):
        return 0
    groups = -(-tiles_n // w_fit)
    return -(-tiles_n // groups)


NGROUP_CONC = {3: 32, 8: 32, 9: 32, 6: 64}   # launch_x: 32 * (1 for 256^2 tiles); conv_gemm_dual_launch: 64
NGROUP_KB = 96
G_NGROUP = geo(3, 3, 61, 64, 2048)            # M = 549: three M rows, the last one a tail


@pytest.mark.parametrize("variant", [3, 6, 8, 9])
def test_n_grouping_ragged_last_group(variant):
    """A 96 KiB budget makes conv_n_group group the eight (dual tile: sixteen) N tiles of a small 1x1 problem by three (six):
    the last group is narrower, tile_order's `width` branch runs."""
    g = G_NGROUP
    bm, bn = TILE[variant]
    width = conv_n_group(1, 1, g.C, 2, g.N, bm, bn, NGROUP_CONC[variant], NGROUP_KB)
    tiles_n = facts(g, BF16, variant)["tiles_n"]
    assert width == (6 if variant == 6 else 3) and 0 < width < tiles_n and tiles_n % width != 0
    run(variant, BF16, g, wide=True, e=dict(bias=chan_bias(g.N)), ngroup_kb=NGROUP_KB)


# ------------------------------------------------------------------ 12. BatchNorm partial statistics from the epilogue
# stats_partial is refused under a forced variant: these cases take the planner's own choice and assert which one it was.
# (id, geometry, hooks, the planner's tile, pixels per partial row)
STATS = [
    ("v1", geo(2, 112, 64, 64, 256), {}, 1, 64),                               # M = 112 * 128: 224 tiles of 128^2
    ("v9", geo(15, 64, 64, 64, 512), {}, 9, 128),                              # M = 240 * 256: 480 tiles of 256^2
    ("v3", geo(15, 64, 64, 64, 512), dict(persist=0), 3, 128),
    ("v4", geo(15, 64, 64, 64, 512, 3, pad=1), {}, 4, 128),
    ("v3-3x3", geo(15, 64, 64, 64, 512, 3, pad=1), dict(sf=0), 3, 128),
]


@functools.lru_cache(maxsize=2)
def stats_problem(g):
    """x and w in -1..1; the reference in f32 on the CPU, exact under the 2^24 bound (float64 would take far longer)."""
    x, w4 = ints((g.B, g.H, g.W, g.C), 7 + g.R, -1, 1), ints((g.N, g.C, g.R, g.S), 8 + g.R, -1, 1)
    bias = chan_bias(g.N)
    assert_exact_bound(x, w4, g.R * g.S * g.C, dict(bias=bias))
    if g.R == 1:
        y = (x.float().view(-1, g.C) @ w4.float().view(g.N, g.C).t()).view(g.B, g.H, g.W, g.N)
    else:
        y = F.conv2d(x.float().permute(0, 3, 1, 2), w4.float(), padding=g.pad).permute(0, 2, 3, 1)
    y = (y + bias.float()).contiguous()
    assert_bf16_exact(y)
    return x, w4, bias, y


@pytest.mark.parametrize("name,g,hooks,variant,pixels", STATS, ids=[r[0] for r in STATS])
def test_batchnorm_partial_statistics(name, g, hooks, variant, pixels):
    """With integer outputs within 2^8 every partial sum (<= 128 * 2^8) and sum of squares (<= 128 * 2^16) is an integer below
    2^24: each partial row equals the integer sums of its pixels, their float64 total equals the column sums of the reference,
    and bn_stats_finalize's mean and biased variance (float64 arithmetic, one rounding to f32) agree with float64 to within
    that one rounding."""
    x, w4, bias, y_ref = stats_problem(g)
    M = g.B * g.H * g.W
    assert M % TILE[variant][0] == 0 and g.N % TILE[variant][1] == 0, "whole tiles only"
    assert pixels * BF16_EXACT ** 2 < EXACT
    xd, wd = x.to(DEV, BF16), gemm_weights(w4).to(DEV, BF16)
    out = torch.full((g.B, g.H, g.W, g.N), NAN, device=DEV, dtype=BF16)
    # (the partial rows are allocated inside ops.conv_gemm, so they cannot be poisoned here: a partial row that is never written is
    # seen only if the memory it got differs from the expected integers -- every row is compared below, none is assumed)
    with forced(-1, **hooks) as timer:
        _, partials, rows = ops.conv_gemm(xd, wd, R=g.R, S=g.S, pad=g.pad, bias=bias.float().to(DEV), out=out, want_stats=True)
        torch.cuda.synchronize()
    assert timer.variants == [variant], f"the planner chose tile {timer.variants}"
    assert rows == M // pixels and tuple(partials.shape) == (rows, 2, g.N)
    assert_same(out.float(), y_ref, f"{name}: output")
    yr = y_ref.double().view(rows, pixels, g.N)
    want = torch.stack([yr.sum(1), (yr * yr).sum(1)], 1)                       # [rows, 2, N], the layout bn_stats_finalize reads
    assert want.abs().max().item() < EXACT
    assert_same(partials, want.float(), f"{name}: partial rows")
    total = partials.double().sum(0).cpu()
    assert torch.equal(total, want.sum(0)), f"{name}: column sums"
    mean, var = ops.bn_stats_finalize(partials, rows, g.N, M)
    mean64 = want[:, 0].sum(0) / M
    var64 = want[:, 1].sum(0) / M - mean64 * mean64
    one_rounding = 2.0 ** -24 * (1 + 2.0 ** -10)       # half an f32 ulp, relative, plus the float64 error of the kernel's own arithmetic
    assert ((mean.double().cpu() - mean64).abs() <= one_rounding * mean64.abs()).all(), f"{name}: mean"
    assert ((var.double().cpu() - var64).abs() <= one_rounding * var64.abs()).all(), f"{name}: biased variance"
