"""Exact-integer tests of the weight-gradient kernels (csrc/wgrad.hip), their split-K paths and, briefly, the forward GEMM.

Operands are small integers (|v| <= 2).  They are exact in bf16 and f32, every product is exact and every partial sum -- in any
order, in an MFMA accumulator, a split-K partial or a reduction kernel -- is an integer below 2^24, so the f32 result has
exactly one correct bit pattern.  Every comparison in this file is ``torch.equal`` against an integer reference computed in
float64 on the CPU: a pixel that is dropped, duplicated or attributed to the wrong tap, a split that is read but never
written, an output element that is never stored are all hard failures, at whatever scale they occur.

The launcher below fills ``gdl_wgrad_args`` as ``ops.conv_wgrad`` does, but owns the workspace and pre-fills it (and, without
``accumulate``, the output) with NaN: what the caching allocator would hide poisons the result.  The split count of every
case comes from ``gdl_conv_wgrad_workspace`` and is asserted, so each case proves which reduction ran (none / the narrow
one / the wide one for >= 16 splits of an unbatched call) and fails loudly when a change of the split rule moves its shape
to another path.  The counts in the tables are those the query reports on an MI355X (256 CUs).
"""

import contextlib
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import _lib, ops  # noqa: E402

DEV = "cuda"
EXACT = 1 << 24                       # every integer of magnitude <= 2^24 is an f32
NAN = float("nan")


# ------------------------------------------------------------------ helpers: operands, bound, references
def ints(shape, seed, lo=-2, hi=2):
    """Seeded integer-valued CPU tensor (float64) with lo <= v <= hi."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g).double()
    assert t.numel() == 0 or (t.min().item() >= lo and t.max().item() <= hi)
    return t


def assert_exact_bound(x, dy, P, dw0=None):
    """max|x| * max|dy| * P + max|dw0| < 2^24: no partial sum of P products, in any order, on top of dw0, leaves the
    integers that f32 holds exactly.  Returns the bound's left-hand side."""
    lhs = x.abs().max().item() * dy.abs().max().item() * P + (0.0 if dw0 is None else dw0.abs().max().item())
    assert lhs < EXACT, f"operands are not exact in f32: {lhs} >= 2^24"
    for t in (x, dy) + (() if dw0 is None else (dw0,)):
        assert torch.equal(t, t.round()), "operands must be integers"
    return lhs


def ref_conv_wgrad(x, dy, R, S, stride, pad, groups=1):
    """Integer reference: x NHWC [B,H,W,C], dy NHWC [B,Ho,Wo,N] (float64) -> dw [N, R*S*(C/groups)] f32 in the kernels' K
    order (r, s, c), through F.conv2d's autograd in float64 (exact on these integers)."""
    assert x.dtype == torch.float64 and dy.dtype == torch.float64
    assert_exact_bound(x, dy, dy.shape[0] * dy.shape[1] * dy.shape[2])
    w = torch.zeros(dy.shape[3], x.shape[3] // groups, R, S, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, stride=stride, padding=pad, groups=groups)
    assert tuple(y.shape[2:]) == tuple(dy.shape[1:3]), (y.shape, dy.shape)
    y.backward(dy.permute(0, 3, 1, 2))
    return w.grad.permute(0, 2, 3, 1).reshape(dy.shape[3], -1).float()


def ref_gemm_wgrad(x, dy):
    """Integer reference of the 1x1 / batched case: x [..., P, C], dy [..., P, N] (float64) -> dw [..., N, C] f32."""
    assert x.dtype == torch.float64 and dy.dtype == torch.float64
    assert_exact_bound(x, dy, x.shape[-2])
    return torch.einsum("...pn,...pc->...nc", dy, x).float()


def assert_same(got, ref, what):
    """torch.equal with a message that says how the result differs."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype == torch.float32, (what, got.shape, ref.shape, got.dtype)
    if torch.equal(got, ref):
        return
    bad = (got != ref) | got.isnan()
    first = bad.nonzero()[0].tolist()
    diff = (got - ref)[bad & ~got.isnan()].abs()
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(got.isnan().sum())} NaN, largest "
                         f"finite difference {diff.max().item() if diff.numel() else 0.0}), first at {first}: "
                         f"got {got[tuple(first)].item()} want {ref[tuple(first)].item()}")


@functools.lru_cache(maxsize=16)
def problem(B, H, W, Cc, N, R, S, stride, pad):
    """(x NHWC, dy NHWC, dw reference) of one convolution geometry, computed once and shared by every kernel's case."""
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    x, dy = ints((B, H, W, Cc), 11 + H * W), ints((B, Ho, Wo, N), 23 + H * W)
    if R == 1 and S == 1 and stride == 1 and pad == 0:
        ref = ref_gemm_wgrad(x.reshape(-1, Cc), dy.reshape(-1, N))
    else:
        ref = ref_conv_wgrad(x, dy, R, S, stride, pad)
    return x, dy, ref


# ------------------------------------------------------------------ helpers: hooks, launcher, split count
@contextlib.contextmanager
def hooks(small=0, v1=0, old=0):
    """Kernel selection through the existing gdl_debug_* hooks; always reset."""
    lib = _lib.load()
    lib.gdl_debug_force_wgrad_small(small)
    lib.gdl_debug_force_wgrad_v1(v1)
    lib.gdl_debug_set_wgrad_old_splits(old)
    try:
        yield
    finally:
        lib.gdl_debug_force_wgrad_small(0)
        lib.gdl_debug_force_wgrad_v1(0)
        lib.gdl_debug_set_wgrad_old_splits(0)


# case name of a kernel -> (operand dtype, gdl_debug_force_wgrad_small, gdl_debug_force_wgrad_v1)
KERNELS = {
    "f32": (torch.float32, 0, 0),       # wgrad_kernel<float>
    "v1": (torch.bfloat16, 0, 1),       # wgrad_kernel<bf16_tag>, the register-transpose kernel
    "tr128": (torch.bfloat16, 3, 0),    # wgrad_tr_kernel, 128^2 tiles, LDS-transposing reads
    "tr256": (torch.bfloat16, 2, 0),    # wgrad_tr256_kernel (N, C >= 256); the hook keeps 3x3 layers off the row segments
    "rows": (torch.bfloat16, 0, 0),     # wgrad_rows_kernel (3x3 / stride 1 / pad 1, W >= 32)
}
KSTEP = {torch.float32: 32, torch.bfloat16: 64}


def rows_seglen(W):
    u, n = (W + 15) // 16, (W + 63) // 64
    return 16 * ((u + n - 1) // n)


def kernel_of(a, small, v1, old):
    """The dispatcher's choice (gdl_conv_wgrad, wgrad_rows_ok, wgrad_tile) for args `a` under the hooks: each case asserts
    that its shape reaches the kernel it is named after."""
    if a.dtype == ops.F32:
        return "f32"
    big = not (small & 1) and a.N >= 256 and a.C >= 256
    rows = (not (small & 2) and (a.R, a.S, a.stride, a.pad) == (3, 3, 1, 1) and a.H == a.Ho and a.W == a.Wo and a.W >= 32
            and a.nz == 1)
    if rows and big and not old:
        seglen = rows_seglen(a.W)
        rows = 5 * seglen * ((a.W + seglen - 1) // seglen) < 6 * a.W and a.N * a.C < 256 * 1024
    if v1:
        return "v1"
    return "rows" if rows else "tr256" if big else "tr128"


def wgrad_args(x4, dy4, dw, *, R, S, stride=1, pad=0, accumulate=False, Cc=None, N=None, nz=1, nz_inner=1,
               in_sZ=(0, 0), dy_sZ=(0, 0), dw_sZ=(0, 0)):
    """gdl_wgrad_args exactly as ops.conv_wgrad fills them (Cc / N and the batch strides as conv_wgrad_grouped / _bwgrad)."""
    x4, dy4 = ops._nhwc4(x4, "wgrad x"), ops._nhwc4(dy4, "wgrad dy")
    assert x4.dtype == dy4.dtype
    a = _lib.WgradArgs()
    a.inp, a.dy, a.dtype = x4.data_ptr(), dy4.data_ptr(), ops.dt(x4)
    a.B, a.H, a.W, a.C = x4.shape[0], x4.shape[1], x4.shape[2], x4.shape[3] if Cc is None else Cc
    a.in_sB, a.in_sH, a.in_sW = x4.stride(0), x4.stride(1), x4.stride(2)
    a.Ho, a.Wo, a.R, a.S, a.stride, a.pad = dy4.shape[1], dy4.shape[2], R, S, stride, pad
    a.N = dy4.shape[3] if N is None else N
    a.dy_sB, a.dy_sH, a.dy_sW = dy4.stride(0), dy4.stride(1), dy4.stride(2)
    a.dw, a.dw_sN, a.accumulate = dw.data_ptr(), dw.stride(-2), int(accumulate)
    a.nz, a.nz_inner = nz, nz_inner
    a.in_sZ0, a.in_sZ1 = in_sZ
    a.dy_sZ0, a.dy_sZ1 = dy_sZ
    a.dw_sZ0, a.dw_sZ1 = dw_sZ
    return a


def splits_of(a):
    """Split count of a call: workspace bytes / (nz * N * R * S * C * 4), where no workspace means one split."""
    nbytes = _lib.load().gdl_conv_wgrad_workspace(C.byref(a))
    per = max(a.nz, 1) * a.N * a.R * a.S * a.C * 4
    assert nbytes % per == 0, (nbytes, per)
    return max(nbytes // per, 1)


def launch(a):
    """Run gdl_conv_wgrad on a NaN-filled workspace of exactly the size the query asks for; returns the split count."""
    lib = _lib.checked()
    nbytes = lib.gdl_conv_wgrad_workspace(C.byref(a))
    ws = torch.full((max(nbytes, 4) // 4,), NAN, device=DEV, dtype=torch.float32)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    lib.gdl_conv_wgrad(C.byref(a), ops._stream())
    torch.cuda.synchronize()
    return splits_of(a)


def split_class(splits):
    return "one" if splits == 1 else "narrow" if splits < 16 else "wide"


def last_split(a, splits, kernel):
    """"empty" / "short" / "ragged" / "full": what the last split of the call holds.  Pixels for the per-tap kernels
    (p_per_split is rounded up to the K-step; "short" = fewer than one K-step), row segments for the row-segment kernel."""
    if kernel == "rows":
        seglen = rows_seglen(a.W)
        total = a.B * a.H * ((a.W + seglen - 1) // seglen)
        per, unit = -(-total // splits), 1
    else:
        total, unit = a.B * a.Ho * a.Wo, KSTEP[torch.float32 if a.dtype == ops.F32 else torch.bfloat16]
        per = -(-(-(-total // splits)) // unit) * unit
    left = total - (splits - 1) * per
    return "empty" if left <= 0 else "short" if kernel != "rows" and left < unit else "ragged" if left < per else "full"


GUARD = 4        # f32 guard columns on each side of a sliced dw


def run_conv_case(kernel, geom, want_splits, *, old=0, accumulate=False, dw_slice=False, dy_slice=False, in_slice=False,
                  in_rows=False, last=None):
    """One convolution weight gradient on `kernel`, compared bit for bit with the integer reference."""
    B, H, W, Cc, N, R, S, stride, pad = geom
    dtype, small, v1 = KERNELS[kernel]
    x, dy, ref = problem(*geom)
    K = R * S * Cc
    if kernel != "rows":               # (the row-segment kernel's K-step is a row segment, whatever P is)
        assert (B * dy.shape[1] * dy.shape[2]) % KSTEP[dtype] != 0, "P must not be a multiple of the K-step"
    xd, dyd = x.to(DEV, dtype), dy.to(DEV, dtype)
    if in_slice or in_rows:            # channel slice of a wider buffer / rows longer than W * C, surrounded by non-zero junk
        wide = torch.full((B, H, W + (3 if in_rows else 0), Cc + (16 if in_slice else 0)), 3.0, device=DEV, dtype=dtype)
        view = wide[:, :, :W, 8:8 + Cc] if in_slice else wide[:, :, :W]
        view.copy_(xd)
        xd = view
    if dy_slice:
        wide_dy = torch.full(tuple(dy.shape[:3]) + (N + 16,), 3.0, device=DEV, dtype=dtype)
        wide_dy[..., 8:8 + N] = dyd
        dyd = wide_dy[..., 8:8 + N]
    dw0 = ints((N, K), 5, -3, 3) if accumulate else None
    assert_exact_bound(x, dy, B * dy.shape[1] * dy.shape[2], dw0)
    buf = torch.full((N, K + (2 * GUARD if dw_slice else 0)), NAN, device=DEV, dtype=torch.float32)
    dw = buf[:, GUARD:GUARD + K] if dw_slice else buf
    if dw_slice:
        buf[:, :GUARD], buf[:, GUARD + K:] = 5.0, -7.0
    if accumulate:
        dw.copy_(dw0)
    before = buf.clone()
    with hooks(small, v1, old):
        a = wgrad_args(xd, dyd, dw, R=R, S=S, stride=stride, pad=pad, accumulate=accumulate)
        assert kernel_of(a, small, v1, old) == kernel, f"this shape does not reach the {kernel} kernel"
        splits = launch(a)
    what = f"{kernel} {geom} splits {splits}"
    print(f"{what}: last split {last_split(a, splits, kernel)}")
    assert splits == want_splits, f"{what}: designed for {want_splits} splits"
    if last is not None:
        assert last_split(a, splits, kernel) == last, f"{what}: last split is {last_split(a, splits, kernel)}, designed {last}"
    assert_same(dw, ref + dw0.float() if accumulate else ref, what)
    if dw_slice:
        assert torch.equal(buf[:, :GUARD].view(torch.int32), before[:, :GUARD].view(torch.int32)), f"{what}: left guard written"
        assert torch.equal(buf[:, GUARD + K:].view(torch.int32), before[:, GUARD + K:].view(torch.int32)), f"{what}: right guard written"
    return splits


def g(B, H, W, Cc, N, R=1, S=None, stride=1, pad=None):
    S = R if S is None else S
    return (B, H, W, Cc, N, R, S, stride, (R // 2 if stride == 1 and R == S else 0) if pad is None else pad)


SMALL, BIG = (72, 40), (264, 320)       # (C, N): off the 64 / 128 / 256 tiles, multiples of 8
PER_TAP = ("f32", "v1", "tr128", "tr256")


def chans(kernel):
    return BIG if kernel == "tr256" else SMALL


# ------------------------------------------------------------------ 1. every kernel at splits == 1
ROWS_ONE = [(2, 3, 32), (1, 5, 33), (3, 1, 36), (2, 3, 72), (1, 5, 100)]   # one segment; ragged; H = 1, B > 1; 48 + 24; 64 + 36


@pytest.mark.parametrize("R", [1, 3], ids=["1x1", "3x3"])
@pytest.mark.parametrize("kernel", PER_TAP)
def test_wgrad_one_split(kernel, R):
    """P = 70 pixels (no multiple of the K-step), H != W, N and C off the tile size: one split, direct store."""
    run_conv_case(kernel, g(2, 5, 7, *chans(kernel), R), 1)                         # splits 1


@pytest.mark.parametrize("B,H,W", ROWS_ONE, ids=[f"rows-splits1-{b}x{h}x{w}" for b, h, w in ROWS_ONE])
def test_wgrad_rows_one_split(B, H, W):
    """Row-segment kernel, fewer than 16 segments: one segment per row, a ragged last segment (33, 36), two unequal segments
    of 16-pixel units (72 -> 48 + 24, 100 -> 64 + 36), H = 1 with B > 1."""
    run_conv_case("rows", g(B, H, W, *SMALL, 3), 1, last="full")                       # splits 1


def test_wgrad_rows_one_split_wide_channels():
    """Row-segment kernel on a layer the 256^2 kernel could take (N, C >= 256, W = 64 unpadded): 4 x 5 tiles of 64."""
    run_conv_case("rows", g(1, 3, 64, 264, 256, 3), 1)                                 # splits 1


# ------------------------------------------------------------------ 2. + 3. split-K: both reductions, ragged / empty last split
# (id, kernel, (B, H, W), R, old-splits hook, splits reported by the workspace query on an MI355X, what the last split holds)
SPLIT_CASES = [
    # f32: "about 1024 blocks" rule capped by P / 256
    ("f32-narrow", "f32", (1, 9, 57), 1, 0, 2, "ragged"),               # P = 513
    ("f32-narrow-3x3", "f32", (1, 9, 57), 3, 0, 2, "ragged"),
    ("f32-narrow-short", "f32", (1, 30, 77), 1, 0, 9, "short"),         # P = 2310: 8 x 288 + 6
    ("f32-narrow-empty", "f32", (1, 42, 61), 1, 0, 10, "empty"),        # P = 2562: 9 x 288 >= P
    ("f32-wide-short", "f32", (2, 46, 47), 1, 0, 16, "short"),          # P = 4324: 15 x 288 + 4
    ("f32-wide-empty", "f32", (2, 41, 50), 1, 0, 16, "empty"),          # P = 4100: 15 x 288 >= P
    # bf16 128^2 kernels: the cost model (it never leaves the last split empty: one split less costs no more), then the old rule
    ("tr128-narrow", "tr128", (3, 11, 33), 1, 0, 2, "ragged"),          # P = 1089
    ("tr128-narrow-3x3", "tr128", (1, 21, 58), 3, 0, 2, "ragged"),      # P = 1218
    ("tr128-narrow-short", "tr128", (3, 29, 53), 1, 0, 9, "short"),     # P = 4611: 8 x 576 + 3
    ("tr128-wide", "tr128", (2, 65, 67), 1, 0, 16, "ragged"),           # P = 8710
    ("tr128-wide-short", "tr128", (3, 43, 67), 1, 0, 16, "short"),      # P = 8643: 15 x 576 + 3
    ("tr128-narrow-empty-oldrule", "tr128", (2, 42, 61), 1, 1, 10, "empty"),   # P = 5124: 9 x 576 >= P
    ("tr128-wide-empty-oldrule", "tr128", (2, 54, 76), 1, 1, 16, "empty"),     # P = 8208: 15 x 576 >= P
    ("v1-narrow", "v1", (3, 11, 33), 1, 0, 2, "ragged"),
    ("v1-narrow-3x3", "v1", (1, 21, 58), 3, 0, 2, "ragged"),
    ("v1-narrow-short", "v1", (3, 29, 53), 1, 0, 9, "short"),
    ("v1-wide", "v1", (2, 65, 67), 1, 0, 16, "ragged"),
    ("v1-wide-short", "v1", (3, 43, 67), 1, 0, 16, "short"),
    ("v1-narrow-empty-oldrule", "v1", (2, 42, 61), 1, 1, 10, "empty"),
    ("v1-wide-empty-oldrule", "v1", (2, 54, 76), 1, 1, 16, "empty"),
    # bf16 256^2 kernel, 2 x 2 tiles
    ("tr256-narrow", "tr256", (1, 25, 41), 1, 0, 2, "ragged"),          # P = 1025
    ("tr256-narrow-3x3", "tr256", (1, 41, 25), 3, 0, 2, "ragged"),
    ("tr256-narrow-short", "tr256", (3, 29, 53), 1, 0, 9, "short"),
    ("tr256-wide", "tr256", (2, 65, 67), 1, 0, 16, "ragged"),
    ("tr256-wide-short", "tr256", (3, 43, 67), 1, 0, 16, "short"),
    ("tr256-narrow-empty-oldrule", "tr256", (2, 42, 61), 1, 1, 10, "empty"),
    ("tr256-wide-empty-oldrule", "tr256", (2, 54, 76), 1, 1, 16, "empty"),
    # row segments: min(512 / tiles, segments / 8) splits; 10 and 18 splits pad the grid to 16 and 24 rows for the XCD grouping
    ("rows-narrow", "rows", (1, 16, 33), 3, 0, 2, "full"),              # 16 segments
    ("rows-narrow-ragged", "rows", (1, 17, 32), 3, 0, 2, "ragged"),     # 17 segments: 9 + 8
    ("rows-narrow-empty", "rows", (3, 27, 32), 3, 0, 10, "empty"),      # 81 segments, 9 per split: 9 x 9 >= 81
    ("rows-wide", "rows", (3, 48, 33), 3, 0, 18, "full"),               # 144 segments
    ("rows-wide-empty", "rows", (3, 43, 32), 3, 0, 16, "empty"),        # 129 segments, 9 per split: 15 x 9 >= 129
    ("rows-wide-two-segments", "rows", (2, 36, 72), 3, 0, 18, "full"),  # 144 segments of 48 + 24 pixels
]


@pytest.mark.parametrize("name,kernel,bhw,R,old,want,last", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_wgrad_split_k(name, kernel, bhw, R, old, want, last):
    """Split-K partials in a NaN-filled workspace, reduced by the narrow (2..15 splits) or the wide (>= 16 splits) kernel."""
    splits = run_conv_case(kernel, g(*bhw, *chans(kernel), R), want, old=old, last=last)
    assert split_class(splits) == name.split("-")[1], f"{name}: {splits} splits take the other reduction"


# ------------------------------------------------------------------ 4. geometry
GEOMETRIES = {
    "k3s2p1-odd": dict(bhw=(2, 7, 9), R=3, stride=2, pad=1),
    "k2s2p0": dict(bhw=(2, 6, 10), R=2, stride=2, pad=0),
    "k8s8-patch-embed": dict(bhw=(1, 16, 24), R=8, stride=8, pad=0),
    "k3p1-on-1x1-map": dict(bhw=(3, 1, 1), R=3, stride=1, pad=1),
    "k3p1-on-2x2-map": dict(bhw=(2, 2, 2), R=3, stride=1, pad=1),
    "k3x1-p1": dict(bhw=(2, 5, 7), R=3, S=1, stride=1, pad=1),       # R != S: gdl_conv_wgrad has no check against it
    "k1x3-p1": dict(bhw=(2, 5, 7), R=1, S=3, stride=1, pad=1),
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
@pytest.mark.parametrize("kernel", PER_TAP)
def test_wgrad_geometry(kernel, name):
    """Strides, padding-dominated maps and non-square filters on every per-tap kernel, one split each."""
    q = GEOMETRIES[name]
    Cc, N = chans(kernel)
    if name == "k8s8-patch-embed" and kernel == "tr256":
        Cc, N = 256, 264                                               # K = 64 C: keep the reference small
    run_conv_case(kernel, g(*q["bhw"], Cc, N, q["R"], q.get("S"), q["stride"], q["pad"]), 1)      # splits 1


# ------------------------------------------------------------------ 5. output protocol
ONE = {k: g(2, 5, 7, *chans(k), 3) for k in PER_TAP} | {"rows": g(1, 5, 33, *SMALL, 3)}
NARROW = {"f32": ((1, 9, 57), 1, 2), "v1": ((3, 11, 33), 1, 2), "tr128": ((3, 11, 33), 1, 2), "tr256": ((1, 25, 41), 1, 2),
          "rows": ((3, 27, 32), 3, 10)}                                 # (B, H, W), R, splits
WIDE = {"f32": ((2, 46, 47), 1, 16), "v1": ((2, 65, 67), 1, 16), "tr128": ((2, 65, 67), 1, 16), "tr256": ((2, 65, 67), 1, 16),
        "rows": ((3, 48, 33), 3, 18)}
ALL_KERNELS = list(KERNELS)


@pytest.mark.parametrize("kernel", ALL_KERNELS)
def test_wgrad_accumulate_one_split(kernel):
    run_conv_case(kernel, ONE[kernel], 1, accumulate=True)


@pytest.mark.parametrize("kernel", ALL_KERNELS)
def test_wgrad_accumulate_narrow_reduction(kernel):
    bhw, R, want = NARROW[kernel]
    run_conv_case(kernel, g(*bhw, *chans(kernel), R), want, accumulate=True)


@pytest.mark.parametrize("kernel", ALL_KERNELS)
def test_wgrad_accumulate_wide_reduction_into_sliced_dw(kernel):
    bhw, R, want = WIDE[kernel]
    run_conv_case(kernel, g(*bhw, *chans(kernel), R), want, accumulate=True, dw_slice=True)


@pytest.mark.parametrize("kernel", ALL_KERNELS)
def test_wgrad_empty_last_split_accumulate_sliced_dw(kernel):
    """An empty last split must contribute zeros (not stale workspace) to an accumulating reduction."""
    if kernel == "rows":
        run_conv_case(kernel, g(3, 27, 32, *SMALL, 3), 10, accumulate=True, dw_slice=True, last="empty")
    elif kernel == "f32":
        run_conv_case(kernel, g(1, 42, 61, *SMALL), 10, accumulate=True, dw_slice=True, last="empty")
    else:
        run_conv_case(kernel, g(2, 42, 61, *chans(kernel)), 10, old=1, accumulate=True, dw_slice=True, last="empty")


@pytest.mark.parametrize("what", ["dw_slice", "dy_slice", "in_slice", "in_rows"])
@pytest.mark.parametrize("kernel,R", [(k, r) for k in PER_TAP for r in (1, 3)] + [("rows", 3)],
                         ids=[f"{k}-{r}x{r}" for k in PER_TAP for r in (1, 3)] + ["rows-3x3"])
def test_wgrad_sliced_operands(kernel, R, what):
    """dw with a row stride above R*S*C (guard columns bit-unchanged), dy and in as channel slices of wider buffers, in with
    a row stride above W*C -- at one split and through the narrow reduction."""
    run_conv_case(kernel, g(*ONE[kernel][:5], R), 1, **{what: True})
    bhw, Rn, want = NARROW[kernel]
    run_conv_case(kernel, g(*bhw, *chans(kernel), Rn), want, **{what: True})


# ------------------------------------------------------------------ 6. batched problems
def grouped_args(xd, dyd, dw, Z, stride):
    c, n = xd.shape[3] // Z, dyd.shape[3] // Z
    return wgrad_args(xd, dyd, dw, R=3, S=3, stride=stride, pad=1, Cc=c, N=n, nz=Z, nz_inner=1, in_sZ=(c, 0), dy_sZ=(n, 0),
                      dw_sZ=(n * 9 * c, 0))


# (dtype, Z, stride, (B, H, W), splits reported by the workspace query on an MI355X)
GROUPED = [
    (torch.bfloat16, 2, 1, (1, 9, 11), 1), (torch.bfloat16, 8, 1, (1, 9, 11), 1), (torch.bfloat16, 2, 2, (1, 9, 11), 1),
    (torch.bfloat16, 8, 2, (1, 9, 11), 1), (torch.float32, 2, 1, (1, 9, 11), 1), (torch.float32, 8, 2, (1, 9, 11), 1),
    (torch.bfloat16, 2, 1, (2, 40, 45), 7), (torch.bfloat16, 8, 1, (2, 40, 45), 7), (torch.bfloat16, 8, 2, (2, 60, 65), 3),
    (torch.float32, 2, 1, (2, 24, 27), 5), (torch.float32, 8, 1, (2, 24, 27), 5), (torch.float32, 2, 2, (2, 40, 45), 3),
]


@pytest.mark.parametrize("dtype,Z,stride,bhw,want", GROUPED,
                         ids=[f"{'bf16' if d == torch.bfloat16 else 'f32'}-Z{z}-s{s}-splits{w}" for d, z, s, _, w in GROUPED])
def test_wgrad_grouped(dtype, Z, stride, bhw, want):
    """ops.conv_wgrad_grouped (nz = Z channel-slice problems in one launch), also where each problem is itself split: the
    narrow reduction then walks nz * splits partials."""
    B, H, W = bhw
    c, n = 16, 24
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, dy = ints((B, H, W, Z * c), 3 + Z), ints((B, Ho, Wo, Z * n), 4 + Z)
    ref = ref_conv_wgrad(x, dy, 3, 3, stride, 1, groups=Z).view(Z, n, 9 * c)
    xd, dyd = x.to(DEV, dtype), dy.to(DEV, dtype)
    dw = torch.full((Z, n, 9 * c), NAN, device=DEV, dtype=torch.float32)
    a = grouped_args(xd, dyd, dw, Z, stride)
    assert kernel_of(a, 0, 0, 0) == ("f32" if dtype == torch.float32 else "tr128")
    splits = launch(a)
    assert splits == want, f"designed for {want} splits, the query gives {splits}"
    assert_same(dw, ref, f"grouped wgrad Z={Z} stride {stride} splits {splits} (NaN-filled workspace)")
    assert_same(ops.conv_wgrad_grouped(xd, dyd, Z=Z, R=3, S=3, stride=stride, pad=1), ref, "ops.conv_wgrad_grouped")


# (dtype, Nq, splits reported by the workspace query on an MI355X)
BWGRAD = [(torch.bfloat16, 77, 1), (torch.float32, 77, 1), (torch.bfloat16, 2100, 4), (torch.float32, 1300, 5)]


@pytest.mark.parametrize("dtype,Nq,want", BWGRAD, ids=[f"{'bf16' if d == torch.bfloat16 else 'f32'}-Nq{n}-splits{w}" for d, n, w in BWGRAD])
def test_wgrad_batched_attention_heads(dtype, Nq, want):
    """ops._bwgrad as attention_bwd calls it for dK = dS^T Q: nz = B * heads, nz_inner = heads, q a slice of the packed qkv
    tensor with the heads interleaved in its channels, dS dense [B, heads, Nq, npad]."""
    B, Hh, hd, npad = 2, 3, 24, 64
    D = Hh * hd
    qkv, dS = ints((B, Nq, 3 * D), 31), ints((B, Hh, Nq, npad), 32)
    q = qkv[..., D:2 * D]
    ref = ref_gemm_wgrad(q.reshape(B, Nq, Hh, hd).permute(0, 2, 1, 3), dS)              # [B, heads, npad, hd]
    qd = qkv.to(DEV, dtype)[..., D:2 * D]
    dSd = dS.to(DEV, dtype)
    dw = torch.full((B, Hh, npad, hd), NAN, device=DEV, dtype=torch.float32)
    sc_z = (Hh * Nq * npad, Nq * npad)
    a = _lib.WgradArgs()                                               # the same fields as ops._bwgrad, for the query
    a.inp, a.dy, a.dtype = qd.data_ptr(), dSd.data_ptr(), ops.dt(qd)
    a.B, a.H, a.W, a.C = 1, 1, Nq, hd
    a.in_sB, a.in_sH, a.in_sW = Nq * qd.stride(1), Nq * qd.stride(1), qd.stride(1)
    a.Ho, a.Wo, a.R, a.S, a.stride, a.pad, a.N = 1, Nq, 1, 1, 1, 0, npad
    a.dy_sB, a.dy_sH, a.dy_sW = Nq * npad, Nq * npad, npad
    a.dw, a.dw_sN, a.accumulate = dw.data_ptr(), hd, 0
    a.nz, a.nz_inner = B * Hh, Hh
    a.in_sZ0, a.in_sZ1 = qd.stride(0), hd
    a.dy_sZ0, a.dy_sZ1 = sc_z
    a.dw_sZ0, a.dw_sZ1 = Hh * npad * hd, npad * hd
    splits = launch(a)
    assert splits == want, f"designed for {want} splits, the query gives {splits}"
    assert_same(dw, ref, f"batched wgrad, {splits} splits (NaN-filled workspace)")
    dw.fill_(NAN)
    ops._bwgrad(qd, qd.stride(1), (qd.stride(0), hd), dSd, npad, sc_z, dw, Nq, hd, npad, B * Hh, Hh)
    torch.cuda.synchronize()
    assert_same(dw, ref, "ops._bwgrad")


# (dtype, (B, H, W), splits of the phase-batched call, splits of ops.convt2x2_wgrad's call; both from the query on an MI355X)
CONVT = [(torch.bfloat16, (2, 5, 7), 1, 1), (torch.float32, (2, 5, 7), 1, 1), (torch.bfloat16, (2, 23, 29), 2, 2),
         (torch.float32, (2, 23, 29), 5, 5)]


@pytest.mark.parametrize("dtype,bhw,want_phases,want_op", CONVT,
                         ids=[f"{'bf16' if d == torch.bfloat16 else 'f32'}-{b}x{h}x{w}" for d, (b, h, w), _, _ in CONVT])
def test_wgrad_conv_transpose_2x2(dtype, bhw, want_phases, want_op):
    """Gradient of a ConvTranspose2d(k 2, s 2) weight against the integer gradient of F.conv_transpose2d, two ways:
    ops.convt2x2_wgrad (ONE 2x2 / stride-2 weight gradient with in = dy, dy = x, then gdl_convt2x2_unpack_grad), and the
    four output phases as a batched call, nz = 4, nz_inner = 2 (the batching of the ConvTranspose forward GEMM: phase
    (py, px) reads dy at rows 2h + py, columns 2w + px through the batch strides)."""
    B, H, W = bhw
    cin, cout = 24, 40
    x, dy = ints((B, H, W, cin), 41), ints((B, 2 * H, 2 * W, cout), 42)
    assert_exact_bound(x, dy, B * H * W)
    w = torch.zeros(cin, cout, 2, 2, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(x.permute(0, 3, 1, 2), w, stride=2).backward(dy.permute(0, 3, 1, 2))
    ref = w.grad.float()                                               # [Cin, Cout, 2, 2]
    xd, dyd = x.to(DEV, dtype), dy.to(DEV, dtype)
    # the call ops.convt2x2_wgrad makes, on poisoned buffers, then the op itself
    dw = torch.full((cin, 4 * cout), NAN, device=DEV, dtype=torch.float32)
    a = wgrad_args(dyd, xd, dw, R=2, S=2, stride=2, pad=0)
    splits = launch(a)
    assert splits == want_op, f"designed for {want_op} splits, the query gives {splits}"
    assert_same(dw.view(cin, 2, 2, cout).permute(0, 3, 1, 2).contiguous(), ref, f"2x2 / stride-2 wgrad, {splits} splits")
    assert_same(ops.convt2x2_wgrad(xd, dyd), ref, "ops.convt2x2_wgrad")
    acc = ints((cin, cout, 2, 2), 43, -3, 3).float()
    assert_same(ops.convt2x2_wgrad(xd, dyd, out=acc.to(DEV), accumulate=True), ref + acc, "ops.convt2x2_wgrad accumulate")
    # nz = 4, nz_inner = 2: dw[py][px][n][c]
    dwp = torch.full((2, 2, cout, cin), NAN, device=DEV, dtype=torch.float32)
    phase0 = dyd[:, 0::2, 0::2]                                        # [B, H, W, Cout] view: rows 2h, columns 2w
    a = wgrad_args(xd, phase0, dwp, R=1, S=1, nz=4, nz_inner=2, dy_sZ=(dyd.stride(1), dyd.stride(2)),
                   dw_sZ=(2 * cout * cin, cout * cin))
    splits = launch(a)
    assert splits == want_phases, f"designed for {want_phases} splits, the query gives {splits}"
    assert_same(dwp, ref.permute(2, 3, 1, 0).contiguous(), f"phase-batched wgrad (nz 4, nz_inner 2), {splits} splits")


# ------------------------------------------------------------------ 7. the forward side
FWD_GEOMETRIES = {"1x1": (1, 1, 0), "3x3-p1": (3, 1, 1), "3x3-s2": (3, 2, 1), "k8s8": (8, 8, 0)}
FWD_KERNELS = {"bf16-variant0": (torch.bfloat16, 0), "bf16-variant1": (torch.bfloat16, 1), "f32-variant0": (torch.float32, 0),
               "f32-variant1": (torch.float32, 1), "f32-planned": (torch.float32, -1)}


@functools.lru_cache(maxsize=4)
def fwd_problem(name):
    R, stride, pad = FWD_GEOMETRIES[name]
    B, H, W = (2, 16, 24) if R == 8 else (2, 9, 11)
    Cc, N = (8, 40) if R == 8 else (72, 40)
    x, w, bias = ints((B, H, W, Cc), 51), ints((N, Cc, R, R), 52), ints((N,), 53, -9, 9)
    lhs = x.abs().max().item() * w.abs().max().item() * R * R * Cc + bias.abs().max().item()
    assert lhs < EXACT
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(xr, w, bias, stride=stride, padding=pad)
    dy = ints(tuple(y.shape), 54)
    y.backward(dy)
    return x, w, bias, y.detach().permute(0, 2, 3, 1).float().contiguous(), dy.permute(0, 2, 3, 1).contiguous(), \
        xr.grad.permute(0, 2, 3, 1).float().contiguous()


@pytest.mark.parametrize("geometry", list(FWD_GEOMETRIES))
@pytest.mark.parametrize("kernel", list(FWD_KERNELS))
def test_conv_gemm_exact(kernel, geometry):
    """ops.conv_gemm with integer operands, an integer bias and f32 output equals the integer reference; M = B*Ho*Wo and
    N = 40 leave tails in both tile dimensions.  Stride-1 geometries: the data gradient through ops.pack_dgrad too."""
    dtype, variant = FWD_KERNELS[kernel]
    R, stride, pad = FWD_GEOMETRIES[geometry]
    x, w, bias, y_ref, dy, dx_ref = fwd_problem(geometry)
    N, Cc = w.shape[0], w.shape[1]
    assert (y_ref.shape[0] * y_ref.shape[1] * y_ref.shape[2]) % 64 != 0 and N % 64 != 0
    xd = x.to(DEV, dtype)
    wm = w.permute(0, 2, 3, 1).reshape(N, -1).contiguous()             # [N, (r, s, c)]
    lib = _lib.load()
    lib.gdl_debug_force_conv_variant(variant)
    try:
        y = ops.conv_gemm(xd, wm.to(DEV, dtype), R=R, S=R, stride=stride, pad=pad, bias=bias.float().to(DEV), out_dtype=torch.float32)
        assert_same(y, y_ref, f"conv_gemm {kernel} {geometry}")
        if stride == 1:
            wd = ops.pack_dgrad(wm.float().to(DEV), N, R * R, Cc, dtype)
            dx = ops.conv_gemm(dy.to(DEV, dtype), wd, R=R, S=R, pad=R - 1 - pad, out_dtype=torch.float32)
            assert_same(dx, dx_ref, f"data gradient {kernel} {geometry}")
    finally:
        lib.gdl_debug_force_conv_variant(-1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("Z,stride", [(2, 1), (8, 2)])
def test_conv_gemm_grouped_exact(dtype, Z, stride):
    """ops.conv_gemm_grouped against F.conv2d(groups=Z) on integers.  Its output has the operands' dtype, so the operands
    are kept in -1..1: |y| <= 9 * 16 = 144 and every integer up to 2^8 is a bf16 value, the bf16 output is exact as well."""
    B, H, W, c, n = 2, 9, 11, 16, 24
    x, w = ints((B, H, W, Z * c), 61, -1, 1), ints((Z * n, c, 3, 3), 62, -1, 1)
    y_ref = F.conv2d(x.permute(0, 3, 1, 2), w, stride=stride, padding=1, groups=Z).permute(0, 2, 3, 1).contiguous()
    assert y_ref.abs().max().item() <= 256          # integers up to 2^8 are bf16 values: the bf16 output is exact too
    wm = w.permute(0, 2, 3, 1).reshape(Z, n, 9 * c).contiguous()
    y = ops.conv_gemm_grouped(x.to(DEV, dtype), wm.to(DEV, dtype), R=3, S=3, stride=stride, pad=1)
    assert y.dtype == dtype
    assert_same(y.float(), y_ref.float(), f"conv_gemm_grouped Z={Z} stride {stride}")
