"""Exact tests of the HBM-bound row and column kernels between the GEMMs of a transformer step: the column sums, LayerScale
backward, LayerNorm backward, softmax backward, depthwise 3x3 + GELU backward and col2im of csrc/transformer_bwd.hip, the
depthwise 3x3 forward (csrc/dwconv.hip, csrc/dwconv_walk.h), the LayerNorm forward (csrc/norm.hip) and add_rows (csrc/elementwise.hip).

Operands are small seeded integers or dyadic rationals.  They are exact in bf16 and f32, every product is exact and every partial
sum -- in any lane, wave, block partial or the final reduction -- stays below 2^24, so each output has one correct bit pattern
and is compared with ``assert_same`` / ``torch.equal`` against a float64 reference.  ``same`` additionally asserts that the
reference is representable in the output dtype, so a bf16 case cannot pass by rounding.  The largest partial sums of every table
are proven in tests/test_rowcol_exact_host.py, which also checks each reference against a naive loop and each table row against
the structure it claims to reach (lane map, empty trailing blocks, batch boundary inside a block, segment tails, block counts,
the nblk clamp) through the plain-Python mirrors of the launchers kept below.

Every output and every workspace is allocated here and pre-filled with NaN; outputs sit in a frame of sentinel values (before,
after, and between the rows of a strided output) that must stay bit-unchanged.  The kernels are called through the C ABI with
these buffers where ``ops.*`` would hide the workspace or the strides.  The partial rows of the workspace are themselves
checked: no NaN in a row the final pass reads, zeros in the rows of blocks that own no rows, and their sum is the reference.

There is no tolerance in this file except the yardstick bound (``check_yard``) of the cases that cannot be exact: LayerNorm on
real-valued rows, LayerNorm's dx where D is no power of two, and GELU with non-zero pre-activations.  The bound follows
tests/test_hip_bn_conditioning.py, but per element: torch's own f32 CPU operator runs on the same stored values; with a
per-element scale s_i that is computed from the float64 reference alone (the magnitudes of the terms that make up element i,
see ``ln_ref`` and the dwconv cases), the yardstick is max_i |torch_i - ref_i| / s_i and the kernel may reach 4 x that (another
summation order) plus one rounding of its output dtype.  Each such case prints kernel error, yardstick and their ratio on a
``ROWCOL`` line.  The bound never depends on what the kernel returned.

LayerNorm's exact family rests on a precondition that the forward kernel itself shows on the device: rows of +1 and -1 in equal
number with eps = 0 and gamma = 1, beta = 0 come back bit for bit, i.e. rsqrtf(1.0f) == 1.0f (test_layernorm_precondition).
Constant rows (value 3, eps = 1e-5) are expected to give beta exactly: 3 D / D is a correctly rounded division.  Both hold on
an MI355X, so nothing had to move to the tolerance family.  Measured there, the kernels' worst error / bound of the yardstick
cases: LayerNorm f32 y 0.27 (random rows), 0.23 (|mean|/std = 30), 0.47 (1000); dx <= 0.32, dgamma <= 0.25, dbeta <= 0.53;
depthwise + GELU forward <= 0.24, backward dpre 0.12, dw9 0.41, db 0.21; bf16 outputs are one bf16 rounding (<= 1.00 of 2^-8).

Two notes on the tables.  The 8200 x 260 f32 column-sum operand is 8.5 MB, the largest tensor here.  col2im's cross of
geometries and maps leaves out the pairs whose kernel is larger than the padded map (8 x 8 on 9 x 7, ...): no convolution has
them, and the host file asserts that nothing else is dropped.
"""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import _lib, ops  # noqa: E402

from test_hip_wgrad_exact import EXACT, assert_same, ints  # noqa: E402

DEV = "cuda"
NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32
DT_ID = {BF16: "bf16", F32: "f32"}
PAIRS = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]
ROUNDING = {F32: 2.0 ** -24, BF16: 2.0 ** -8}
GUARD = 64                             # sentinel elements in front of and behind every framed buffer
SENT = -12345.0


# ------------------------------------------------------------------ mirrors of the launchers (checked by the host file)
def row_blocks(rows):
    """transformer_bwd.hip row_blocks: clamp(rows / 16, 1, 512)."""
    return min(max(rows // 16, 1), 512)


def partition(units, nblk):
    """(per, first block that owns nothing): block b takes units [per b, min(per (b + 1), units))."""
    per = -(-units // nblk)
    return per, min(-(-units // per), nblk)


def col_lanes(C):
    """col_map: lanes on one row (4 channels per lane)."""
    return 64 if C > 128 else 32 if C > 64 else 16 if C > 32 else 8 if C > 16 else 4


def dw_lanes(C):
    """dwconv_gelu_bwd_kernel's own map."""
    return 64 if C > 128 else 32 if C > 64 else 16


def ln_lanes(D):
    """LayerNorm forward and backward: (lanes on one row, float4 vectors per lane)."""
    vpl = -(-D // 256)
    vpl = 1 if vpl <= 1 else 2 if vpl <= 2 else 4
    return (64 if D > 128 else 32 if D > 64 else 16), vpl


def seg_len(W):
    return W if W <= 32 else 32


def segments(W):
    """[(x0, x1)] of one image row, as gdldw::seg_of cuts it."""
    s = seg_len(W)
    return [(x0, min(x0 + s, W)) for x0 in range(0, W, s)]


def dw_fwd_blocks(B, H, W, C):
    """(256-thread blocks that hold a thread with work, launched grid = that rounded up to the 8 XCDs)."""
    total = B * len(segments(W)) * H * (C // 4)
    nb = -(-total // 256)
    return nb, -(-nb // 8) * 8


def dw_bwd_blocks(B, H, W, C):
    """(nblk of gdl_dwconv3x3_gelu_bwd, row_blocks(P) that sizes the workspace, items)."""
    items = B * len(segments(W)) * H
    nsub = 64 // dw_lanes(C)
    rb = row_blocks(B * H * W)
    return min(rb, -(-items // (4 * nsub))), rb, items


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


# ------------------------------------------------------------------ buffers, comparisons
def LIB():
    return _lib.checked()


def P(t):
    return ops._p(t)


def dev(t, dtype=F32):
    return t.to(dtype).to(DEV).contiguous()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


class Framed:
    """A tensor of `full_shape` whose part `index` is the kernel's output (NaN-filled); everything else, and GUARD elements on
    both sides of the allocation, holds a sentinel that ``check`` wants bit-unchanged."""

    def __init__(self, full_shape, dtype, index=Ellipsis, fill=None):
        n = math.prod(full_shape)
        self.buf = torch.full((n + 2 * GUARD,), SENT, device=DEV, dtype=dtype)
        self.full_shape, self.index = tuple(full_shape), index
        self.view = self.buf[GUARD:GUARD + n].view(self.full_shape)[index]
        if fill is None:
            self.view.fill_(NAN)
        else:
            self.view.copy_(fill)

    def check(self, what):
        c = self.buf.clone()
        c[GUARD:c.numel() - GUARD].view(self.full_shape)[self.index] = SENT
        assert torch.equal(bits(c).cpu(), bits(torch.full_like(c, SENT)).cpu()), f"{what}: a sentinel around the output changed"


def same(got, ref, what):
    """Bit-exact comparison of a kernel output (f32 or bf16) with a float64 reference that its dtype must hold exactly."""
    assert ref.dtype == torch.float64
    assert torch.equal(ref.to(got.dtype).double(), ref), f"{what}: the reference is not representable in {got.dtype}"
    assert ref.abs().max().item() < EXACT
    assert_same(got.float(), ref.float(), what)


def check_yard(got, ref, t32, scale, out_dtype, what):
    """The yardstick bound of the module docstring.  ref, scale: float64 (CPU); t32: torch's f32 result on the same values."""
    s = scale.double().clamp_min(1e-300)
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{what}: not finite"
    ek, et = ((got - ref).abs() / s).max().item(), ((t32.double() - ref).abs() / s).max().item()
    bound = 4 * et + ROUNDING[out_dtype]
    print(f"ROWCOL {what}: kernel {ek:.3e} torch f32 {et:.3e} bound {bound:.3e} ratio {ek / bound:.3f}")
    assert ek <= bound, f"{what}: per-element error {ek:.3e} > {bound:.3e} (torch f32: {et:.3e})"
    return ek / bound


def owned_ws(rows, Cc, planes):
    nbytes = _lib.load().gdl_colreduce_workspace(rows, Cc, planes)
    assert nbytes == row_blocks(rows) * planes * Cc * 4, "row_blocks mirror out of date"
    return torch.full((nbytes // 4,), NAN, device=DEV, dtype=F32), nbytes


def check_partials(ws, n_rows_ws, width, units, nblk, ref, what):
    """ws: [n_rows_ws][width] partial rows of which the final pass reads the first nblk; `units` rows / items are dealt to them.
    No NaN in a row that is read, zeros in the rows of blocks that own nothing, the rows' sum is `ref` (float64, `width`)."""
    part = ws.cpu().view(n_rows_ws, width)
    per, first_empty = partition(units, nblk)
    used = part[:nblk]
    assert not used.isnan().any(), f"{what}: a partial row that the final pass reads was not written"
    assert (used[first_empty:] == 0).all(), f"{what}: the partial row of a block without rows is not zero"
    assert part[nblk:].isnan().all(), f"{what}: a partial row beyond the grid was written"
    assert_same(used.double().sum(0).float(), ref.reshape(-1).float(), what + " (sum of partials)")
    return nblk - first_empty


# ================================================================== 1. column sums
# every partial sum is at most 2 * 8200 (+ 100 preset) -- proven in the host file
COLSUM_C = (4, 16, 20, 32, 64, 96, 128, 132, 160, 256, 260, 320, 768)
COLSUM_ROWS = (1, 3, 6, 15, 16, 17, 33, 47, 289, 300)          # crossed with every C; 289: the first row count with an empty block
COLSUM_BIG = [(8191, 4), (8191, 96), (8192, 4), (8192, 32), (8192, 96), (8200, 32), (8200, 260)]
COLSUM_LAYOUT_C = (4, 20, 64, 96, 260)                          # one C per lane map


@functools.lru_cache(maxsize=None)
def colsum_operand(Cc):
    x = ints((max(COLSUM_ROWS), Cc), 100 + Cc)
    return x, x.cumsum(0)


def run_colsum(x2, out, accumulate, what, ref):
    rows, Cc = x2.shape
    ws, nbytes = owned_ws(rows, Cc, 1)
    LIB().gdl_colsum(P(x2), ops.dt(x2), rows, Cc, x2.stride(0), P(out.view), int(accumulate), P(ws), nbytes, ops._stream())
    torch.cuda.synchronize()
    same(out.view, ref, what)
    out.check(what)
    return ws


@pytest.mark.parametrize("dtype", [F32, BF16], ids=DT_ID.get)
@pytest.mark.parametrize("Cc", COLSUM_C)
def test_colsum_dense(Cc, dtype):
    x, cum = colsum_operand(Cc)
    xd = dev(x, dtype)
    for rows in COLSUM_ROWS:
        what = f"colsum {DT_ID[dtype]} rows={rows} C={Cc}"
        ws = run_colsum(xd[:rows], Framed((Cc,), F32), False, what, cum[rows - 1])
        check_partials(ws, row_blocks(rows), Cc, rows, row_blocks(rows), cum[rows - 1], what)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=DT_ID.get)
@pytest.mark.parametrize("rows,Cc", COLSUM_BIG)
def test_colsum_many_rows(rows, Cc, dtype):
    x = ints((rows, Cc), 7 + rows + Cc)
    ref = x.sum(0)
    what = f"colsum {DT_ID[dtype]} rows={rows} C={Cc}"
    ws = run_colsum(dev(x, dtype), Framed((Cc,), F32), False, what, ref)
    empty = check_partials(ws, row_blocks(rows), Cc, rows, row_blocks(rows), ref, what)
    assert empty == {8191: 29, 8192: 0, 8200: 29}[rows]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=DT_ID.get)
@pytest.mark.parametrize("Cc", COLSUM_LAYOUT_C)
def test_colsum_layouts_and_accumulate(Cc, dtype):
    for rows in (3, 17, 47):
        g = ints((rows, 3, Cc), 31 * rows + Cc)                       # production: the class-token gradient g[:, 0, :]
        gd = dev(g, dtype)
        what = f"colsum {DT_ID[dtype]} g[:, 0, :] B={rows} C={Cc}"
        assert gd[:, 0, :].stride(0) == 3 * Cc
        run_colsum(gd[:, 0, :], Framed((Cc,), F32), False, what, g[:, 0, :].sum(0))
        wide = ints((rows, Cc + 12), 37 * rows + Cc)                  # a channel slice: row stride > C
        wd = dev(wide, dtype)
        run_colsum(wd[:, 4:4 + Cc], Framed((Cc,), F32), False, what + " slice", wide[:, 4:4 + Cc].sum(0))
        out0 = ints((Cc,), 41 * rows + Cc, -100, 100)
        run_colsum(wd[:, 8:8 + Cc], Framed((Cc,), F32, fill=dev(out0)), True, what + " accumulate", out0 + wide[:, 8:8 + Cc].sum(0))


# ================================================================== 2. LayerScale / DropPath backward
LS_C = (4, 20, 64, 96, 132, 260, 768)            # one per lane map, and three channel blocks
LS_BN = [(3, 1), (3, 5), (3, 11), (3, 100)]      # (3, 11): 33 rows in 2 blocks of 17, block 0 spans batches 0 and 1
LS_BIG = (3, 2731, 32)                           # 8193 rows: 512 blocks of 17 of which the last 30 own nothing
LS_SCALES = (0.0, 1.0, 1.25, 2.0)
LS_FORMS = ("gamma", "gamma+scale", "scale", "cast")


def ls_case(B, N, Cc, form):
    seed = 1000 * B + 10 * N + Cc + len(form)
    g = 4 * ints((B, N, Cc), seed)                                   # multiples of 4: g * 1.25 is an integer
    z, gamma = ints((B, N, Cc), seed + 1, -3, 3), ints((Cc,), seed + 2, -3, 3)
    s = torch.tensor([LS_SCALES[(b + Cc // 4 + N) % 4] for b in range(B)], dtype=torch.float64)
    if form in ("gamma", "cast"):
        s = None
    if form in ("scale", "cast"):
        z = gamma = None
    gs = g if s is None else g * s[:, None, None]
    dz = gs if gamma is None else gs * gamma
    dgamma = None if gamma is None else (gs * z).sum((0, 1))
    return g, z, gamma, s, dz, dgamma


def run_layerscale(g, z, gamma, s, dz_ref, dgamma_ref, z_dtype, dz_dtype, what, dgamma0=None):
    B, N, Cc = g.shape
    rows = B * N
    dz = Framed((B, N, Cc), dz_dtype)
    zd = None if z is None else dev(z, z_dtype)
    gd, gam, sd = dev(g), None if gamma is None else dev(gamma), None if s is None else dev(s)
    ws, nbytes, dg = None, 0, None
    if gamma is not None:
        ws, nbytes = owned_ws(rows, Cc, 1)
        dg = Framed((Cc,), F32, fill=None if dgamma0 is None else dev(dgamma0))
    LIB().gdl_layerscale_bwd(P(gd), P(zd), ops.dt(z_dtype), P(gam), P(sd), rows, N, Cc, P(dz.view), ops.dt(dz_dtype),
                             P(None if dg is None else dg.view), int(dgamma0 is not None), P(ws), nbytes, ops._stream())
    torch.cuda.synchronize()
    same(dz.view, dz_ref, what + " dz")
    dz.check(what + " dz")
    if gamma is not None:
        same(dg.view, dgamma_ref if dgamma0 is None else dgamma_ref + dgamma0, what + " dgamma")
        dg.check(what + " dgamma")
        check_partials(ws, row_blocks(rows), Cc, rows, row_blocks(rows), dgamma_ref, what)


@pytest.mark.parametrize("form", LS_FORMS)
@pytest.mark.parametrize("Cc", LS_C)
def test_layerscale_bwd(Cc, form):
    for B, N in LS_BN:
        g, z, gamma, s, dz, dgamma = ls_case(B, N, Cc, form)
        for z_dtype, dz_dtype in (PAIRS if gamma is not None else [(F32, F32), (F32, BF16)]):
            what = f"layerscale_bwd {form} z={DT_ID[z_dtype]} dz={DT_ID[dz_dtype]} B={B} N={N} C={Cc}"
            run_layerscale(g, z, gamma, s, dz, dgamma, z_dtype, dz_dtype, what)
    g, z, gamma, s, dz, dgamma = ls_case(3, 11, Cc, form)
    if gamma is not None:                                            # accumulate: once per lane map and form
        run_layerscale(g, z, gamma, s, dz, dgamma, BF16, F32, f"layerscale_bwd {form} accumulate C={Cc}",
                       dgamma0=ints((Cc,), Cc, -100, 100))


@pytest.mark.parametrize("form", LS_FORMS)
def test_layerscale_bwd_many_rows(form):
    B, N, Cc = LS_BIG
    g, z, gamma, s, dz, dgamma = ls_case(B, N, Cc, form)
    run_layerscale(g, z, gamma, s, dz, dgamma, BF16, BF16, f"layerscale_bwd {form} B={B} N={N} C={Cc}")


# ================================================================== 3. LayerNorm forward and backward
LN_D = (4, 32, 64, 68, 96, 128, 132, 160, 256, 260, 320, 512, 516, 768, 1024)
LN_ROWS = (1, 5, 6, 37, 300)
LN_BIG = (8200, 32)
LN_KINDS = ("random", "kappa30", "kappa1000", "const3")
LN_EPS = 1e-5


def pm_rows(rows, D, seed):
    """rows of +1 and -1 in equal number, in a seeded order"""
    gen = torch.Generator().manual_seed(seed)
    base = torch.cat([torch.ones(D // 2), -torch.ones(D // 2)]).double()
    return base[torch.rand(rows, D, generator=gen).argsort(1)]


def real_rows(rows, D, kind, seed):
    """f32-representable rows (float64): standard normal, |mean| / std = 30 or 1000 (sample statistics), or the constant 3"""
    if kind == "const3":
        return torch.full((rows, D), 3.0, dtype=torch.float64)
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, D, generator=gen, dtype=torch.float64)
    if kind != "random":
        z = (z - z.mean(1, keepdim=True)) / z.std(1, unbiased=False, keepdim=True) + float(kind[5:])
    return z.float().double()


def ln_ref(x, gamma, beta, eps, dy, dres=None):
    """float64 LayerNorm forward and backward in the kernels' formulation, with the per-element scales of the yardstick bound:
    the magnitudes of the terms of each element, where a normalised value counts as at least 1 (an error of the row mean moves
    every xhat of the row by the same absolute amount)."""
    D = x.shape[1]
    mu = x.sum(1, keepdim=True) / D
    var = ((x - mu) ** 2).sum(1, keepdim=True) / D
    rstd = 1.0 / (var + eps).sqrt()                 # sqrt and the division are correctly rounded: exactly 1 for var = 1, eps = 0
    xhat = (x - mu) * rstd
    big = xhat.abs().clamp_min(1.0)
    g = dy * gamma
    mg, mgx = g.sum(1, keepdim=True) / D, (g * xhat).sum(1, keepdim=True) / D
    dx = rstd * (g - mg - xhat * mgx)
    s_dx = rstd * (g.abs() + g.abs().mean(1, keepdim=True) + big * (g * xhat).abs().mean(1, keepdim=True))
    if dres is not None:
        dx, s_dx = dx + dres, s_dx + dres.abs()
    return dict(y=xhat * gamma + beta, dx=dx, dgamma=(dy * xhat).sum(0), dbeta=dy.sum(0), xhat=xhat,
                s_y=gamma.abs() * big + beta.abs(), s_dx=s_dx, s_dgamma=(dy.abs() * big).sum(0), s_dbeta=dy.abs().sum(0))


def ln_torch32(x, gamma, beta, eps, dy, dres=None):
    """torch's own f32 CPU LayerNorm, forward and autograd, on the same stored values"""
    xr, g, b = x.float().requires_grad_(True), gamma.float().requires_grad_(True), beta.float().requires_grad_(True)
    y = F.layer_norm(xr, (x.shape[1],), g, b, eps)
    y.backward(dy.float())
    return dict(y=y.detach(), dx=xr.grad if dres is None else xr.grad + dres.float(), dgamma=g.grad, dbeta=b.grad)


def run_ln_fwd(x, gamma, beta, eps, out_dtype, strided):
    """-> y (device, out_dtype); x is passed as a column slice of a wider tensor when `strided`"""
    rows, D = x.shape
    xw = torch.full((rows, D + (12 if strided else 0)), NAN, device=DEV, dtype=F32)
    xv = xw[:, 4:4 + D] if strided else xw
    xv.copy_(x)
    y = Framed((rows, D), out_dtype)
    gd, bd = dev(gamma), dev(beta)                  # named: a temporary would be freed, and its memory reused, before the launch
    LIB().gdl_layernorm_fwd(P(xv), xv.stride(0), P(gd), P(bd), P(y.view), ops.dt(out_dtype), rows, D, eps,
                            ops._stream())
    torch.cuda.synchronize()
    y.check(f"layernorm_fwd rows={rows} D={D}")
    return y.view


def run_ln_bwd(x, dy, gamma, eps, dy_dtype, dres, strided, acc0=None):
    """-> (dx, dgamma, dbeta, ws); strided: x a column slice, dres and dx with row strides of their own"""
    rows, D = x.shape
    pad = (12, 4, 20) if strided else (0, 0, 0)
    xw = torch.full((rows, D + pad[0]), NAN, device=DEV, dtype=F32)
    xv = xw[:, 4:4 + D] if strided else xw
    xv.copy_(x)
    rv = None
    if dres is not None:
        rw = torch.full((rows, D + pad[1]), NAN, device=DEV, dtype=F32)
        rv = rw[:, :D]
        rv.copy_(dres)
    dx = Framed((rows, D + pad[2]), F32, index=(slice(None), slice(8, 8 + D)) if strided else Ellipsis)
    dg = Framed((D,), F32, fill=None if acc0 is None else dev(acc0[0]))
    db = Framed((D,), F32, fill=None if acc0 is None else dev(acc0[1]))
    ws, nbytes = owned_ws(rows, D, 2)
    dyd, gd = dev(dy, dy_dtype), dev(gamma)
    LIB().gdl_layernorm_bwd(P(xv), xv.stride(0), P(dyd), ops.dt(dy_dtype), P(gd), P(rv),
                            0 if rv is None else rv.stride(0), P(dx.view), dx.view.stride(0), rows, D, eps, P(dg.view), P(db.view),
                            int(acc0 is not None), P(ws), nbytes, ops._stream())
    torch.cuda.synchronize()
    what = f"layernorm_bwd rows={rows} D={D}"
    dx.check(what + " dx"), dg.check(what + " dgamma"), db.check(what + " dbeta")
    return dx.view, dg.view, db.view, ws


@functools.lru_cache(maxsize=None)
def rsqrt_of_one_is_one():
    """the exact family's precondition, shown by the forward kernel itself"""
    ok = True
    for D in (4, 64, 128, 320, 1024):
        x = pm_rows(6, D, D)
        y = ops.layernorm(dev(x), torch.ones(D, device=DEV), torch.zeros(D, device=DEV), 0.0, F32)
        ok = ok and torch.equal(bits(y).cpu(), bits(x.float()))
    return ok


def test_layernorm_precondition():
    assert rsqrt_of_one_is_one(), "rsqrtf(1.0f) != 1.0f on this device: the exact LayerNorm family has no footing"


def ln_exact_operands(rows, D):
    x = pm_rows(rows, D, 3 * rows + D)
    gamma, beta = ints((D,), D + 1, -3, 3), ints((D,), D + 2, -8, 8)
    dy, dres = ints((rows, D), rows + D + 3), ints((rows, D), rows + D + 4)
    return x, gamma, beta, dy, dres


def ln_exact_case(rows, D, strided, accumulate):
    assert rsqrt_of_one_is_one()
    x, gamma, beta, dy, dres = ln_exact_operands(rows, D)
    ref = ln_ref(x, gamma, beta, 0.0, dy, dres)
    t32 = None
    for out_dtype in (F32, BF16):
        same(run_ln_fwd(x, gamma, beta, 0.0, out_dtype, strided), ref["y"], f"layernorm_fwd exact {DT_ID[out_dtype]} rows={rows} D={D}")
    acc0 = (ints((D,), D + 5, -100, 100), ints((D,), D + 6, -100, 100)) if accumulate else None
    for dy_dtype in (F32, BF16):
        what = f"layernorm_bwd exact dy={DT_ID[dy_dtype]} rows={rows} D={D} strided={strided} accumulate={accumulate}"
        dx, dg, db, ws = run_ln_bwd(x, dy, gamma, 0.0, dy_dtype, dres, strided, acc0)
        same(dg, ref["dgamma"] + (0 if acc0 is None else acc0[0]), what + " dgamma")
        same(db, ref["dbeta"] + (0 if acc0 is None else acc0[1]), what + " dbeta")
        nblk = row_blocks(rows)
        check_partials(ws, nblk, 2 * D, rows, nblk, torch.cat([ref["dgamma"], ref["dbeta"]]), what)
        if D & (D - 1) == 0:                       # both row means are exact
            same(dx, ref["dx"], what + " dx")
        else:
            t32 = t32 or ln_torch32(x, gamma, beta, 0.0, dy, dres)
            check_yard(dx, ref["dx"], t32["dx"], ref["s_dx"], F32, what + " dx")


@pytest.mark.parametrize("D", LN_D)
def test_layernorm_exact(D):
    for i, rows in enumerate(LN_ROWS):
        ln_exact_case(rows, D, strided=i % 2 == 1, accumulate=i % 3 == 1)


def test_layernorm_exact_many_rows():
    ln_exact_case(*LN_BIG, strided=True, accumulate=True)


def ln_real_operands(rows, D, kind):
    gen = torch.Generator().manual_seed(rows + 7 * D + len(kind))
    x = real_rows(rows, D, kind, rows + D)
    gamma, beta = (torch.randn(D, generator=gen) + 1).double(), torch.randn(D, generator=gen).double()
    dy, dres = torch.randn(rows, D, generator=gen), torch.randn(rows, D, generator=gen).double()
    return x, gamma, beta, dy, dres


@pytest.mark.parametrize("kind", LN_KINDS)
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_yardstick(D, kind):
    rows = 37
    strided = accumulate = kind in ("random", "kappa1000")
    x, gamma, beta, dy32, dres = ln_real_operands(rows, D, kind)
    for dt_ in (F32, BF16):                        # the forward's output dtype and the backward's dy dtype
        dy = dy32.to(dt_).double()                 # the stored values
        ref, t32 = ln_ref(x, gamma, beta, LN_EPS, dy, dres), ln_torch32(x, gamma, beta, LN_EPS, dy, dres)
        what = f"layernorm {kind} {DT_ID[dt_]} rows={rows} D={D}"
        y = run_ln_fwd(x, gamma, beta, LN_EPS, dt_, strided)
        if kind == "const3":
            assert torch.equal(y.cpu(), beta.float().to(dt_).expand(rows, D)), what + ": a constant row must give beta exactly"
        check_yard(y, ref["y"], t32["y"], ref["s_y"], dt_, what + " y")
        gen = torch.Generator().manual_seed(D)
        acc0 = (torch.randn(D, generator=gen).double(), torch.randn(D, generator=gen).double()) if accumulate else (0.0, 0.0)
        dx, dg, db, _ = run_ln_bwd(x, dy, gamma, LN_EPS, dt_, dres, strided, acc0 if accumulate else None)
        check_yard(dx, ref["dx"], t32["dx"], ref["s_dx"], F32, what + " dx")
        a0 = [torch.as_tensor(a, dtype=torch.float64) for a in acc0]
        check_yard(dg, ref["dgamma"] + a0[0], t32["dgamma"].double() + a0[0], ref["s_dgamma"] + a0[0].abs(), F32, what + " dgamma")
        check_yard(db, ref["dbeta"] + a0[1], t32["dbeta"].double() + a0[1], ref["s_dbeta"] + a0[1].abs(), F32, what + " dbeta")


# ================================================================== 4. depthwise 3x3 forward
DW_W = (1, 2, 3, 4, 31, 32, 33, 34, 35, 64, 65, 70)
DW_H = (1, 2, 3, 5)
DW_C = (4, 32, 64, 68, 128, 256, 260, 320)
# forward blocks with work -> (B, H, W, C): one block, 7 (a padded grid of 8), 8 (no padding), 9 and 17 (two per XCD, padded)
DW_BLOCKS = {1: (1, 1, 1, 4), 7: (2, 5, 64, 320), 8: (2, 5, 70, 256), 9: (2, 5, 70, 288), 17: (2, 5, 70, 560)}
DW_DENSE = ([(1 + i % 2, DW_H[i % 4], W, DW_C[i % 8]) for i, W in enumerate(DW_W)]
            + [(2 - i % 2, DW_H[(i + 2) % 4], W, DW_C[(i + 3) % 8]) for i, W in enumerate(DW_W)] + list(DW_BLOCKS.values()))
# basis shapes (B, H, W, C): every segment boundary of a 70-wide row, a 2-pixel tail, single row / column / pixel
DW_BASIS = [(2, 3, 70, 4), (1, 2, 65, 68), (1, 5, 34, 32), (1, 1, 33, 4), (2, 5, 1, 4), (1, 1, 1, 4), (1, 3, 2, 260)]


def basis_pixels(H, W):
    xs = sorted({x for x in (0, 31, 32, 33, 63, 64, W - 1) if x < W})
    return [(y, x) for y in sorted({0, H - 1}) for x in xs]


def w9_basis(Cc):
    return torch.arange(1, 10, dtype=torch.float64)[:, None].expand(9, Cc).contiguous()


def ref_dwconv(u, w9, bias):
    """u NHWC float64, w9 [9, C] with tap t = 3 r + s on u[y + r - 1, x + s - 1] -> NHWC float64"""
    Cc = u.shape[3]
    w4 = w9.t().reshape(Cc, 1, 3, 3)
    return F.conv2d(u.permute(0, 3, 1, 2), w4, bias, padding=1, groups=Cc).permute(0, 2, 3, 1).contiguous()


def shifted(u, r, s):
    """u[b, y + r - 1, x + s - 1, c], zero outside the image"""
    B, H, W, Cc = u.shape
    return F.pad(u, (0, 0, 1, 1, 1, 1))[:, r:r + H, s:s + W]


def run_dwconv(u, w9, bias, gelu, in_dtype, out_dtype, what):
    B, H, W, Cc = u.shape
    out = Framed((B, H, W, Cc), out_dtype)
    ud, wd, bd = dev(u, in_dtype), dev(w9), dev(bias)
    LIB().gdl_dwconv3x3(P(ud), ops.dt(in_dtype), B, H, W, Cc, P(wd), P(bd), int(gelu), P(out.view),
                        ops.dt(out_dtype), ops._stream())
    torch.cuda.synchronize()
    out.check(what)
    return out.view


@pytest.mark.parametrize("B,H,W,Cc", DW_BASIS)
def test_dwconv_basis(B, H, W, Cc):
    w9, zero = w9_basis(Cc), torch.zeros(Cc, dtype=torch.float64)
    amp = 1.0 + torch.arange(Cc, dtype=torch.float64) % 3
    for k, (y0, x0) in enumerate(basis_pixels(H, W)):
        u = torch.zeros(B, H, W, Cc, dtype=torch.float64)
        u[B - 1, y0, x0] = amp
        ref = ref_dwconv(u, w9, zero)
        for in_dtype, out_dtype in ([PAIRS[k % 4]] if Cc > 4 else PAIRS):
            what = f"dwconv basis {DT_ID[in_dtype]}->{DT_ID[out_dtype]} {B}x{H}x{W}x{Cc} one-hot at ({y0}, {x0})"
            same(run_dwconv(u, w9, zero, False, in_dtype, out_dtype, what), ref, what)


@pytest.mark.parametrize("B,H,W,Cc", DW_DENSE)
def test_dwconv_dense(B, H, W, Cc):
    seed = 1000 * W + 10 * H + Cc
    u, w9, bias = ints((B, H, W, Cc), seed, -3, 3), ints((9, Cc), seed + 1, -3, 3), ints((Cc,), seed + 2, -8, 8)
    ref = ref_dwconv(u, w9, bias)
    for in_dtype, out_dtype in PAIRS:
        what = f"dwconv dense {DT_ID[in_dtype]}->{DT_ID[out_dtype]} {B}x{H}x{W}x{Cc}"
        same(run_dwconv(u, w9, bias, False, in_dtype, out_dtype, what), ref, what)
    zero9, zero = torch.zeros(9, Cc, dtype=torch.float64), torch.zeros(Cc, dtype=torch.float64)
    what = f"dwconv gelu of zero {B}x{H}x{W}x{Cc}"
    same(run_dwconv(u, zero9, zero, True, BF16, BF16, what), torch.zeros_like(u), what)


def dw_real_operands(B, H, W, Cc, dtype):
    gen = torch.Generator().manual_seed(B + 3 * H + 5 * W + 7 * Cc)
    u = torch.randn(B, H, W, Cc, generator=gen).to(dtype).double()
    w9, bias = (torch.randn(9, Cc, generator=gen) * 0.4).double(), (torch.randn(Cc, generator=gen) * 0.2).double()
    dy = torch.randn(B, H, W, Cc, generator=gen).to(dtype).double()
    s_pre = sum(shifted(u, t // 3, t % 3).abs() * w9[t].abs() for t in range(9)) + bias.abs()
    return u, w9, bias, dy, s_pre


@pytest.mark.parametrize("B,H,W,Cc", [(2, 3, 33, 68), (1, 5, 70, 4), (2, 2, 35, 260)])
def test_dwconv_gelu_yardstick(B, H, W, Cc):
    """y = gelu(pre): |dy/dpre| <= 1.13, so the terms of pre (sum |u w| + |bias|) are the per-element scale"""
    for in_dtype, out_dtype in PAIRS:
        u, w9, bias, _, s_pre = dw_real_operands(B, H, W, Cc, in_dtype)
        ref = F.gelu(ref_dwconv(u, w9, bias))
        t32 = F.gelu(ref_dwconv(u.float(), w9.float(), bias.float()))
        what = f"dwconv+gelu {DT_ID[in_dtype]}->{DT_ID[out_dtype]} {B}x{H}x{W}x{Cc}"
        check_yard(run_dwconv(u, w9, bias, True, in_dtype, out_dtype, what), ref, t32, s_pre, out_dtype, what)


# ================================================================== 5. depthwise 3x3 + GELU backward
# (B, H, W, C): the forward's ladder thinned; the last three have row_blocks(P) <= ceil(items / (4 nsub)) (clamp inactive)
DWB_SHAPES = [(2, 3, 70, 4), (1, 2, 65, 68), (1, 5, 34, 32), (2, 5, 35, 128), (2, 5, 64, 256), (1, 3, 33, 260), (2, 2, 31, 320),
              (1, 1, 32, 64), (2, 5, 3, 4), (1, 1, 1, 4), (2, 5, 1, 260), (2, 5, 2, 320), (2, 3, 4, 132)]
DWB_BASIS = [(2, 3, 70, 4), (1, 2, 65, 68), (1, 3, 34, 132)]


def ref_dw_bwd(u, dpre):
    """dw9[t][c] = sum dpre[p] u[p + tap t], db[c] = sum dpre[p]  (float64)"""
    return torch.stack([(dpre * shifted(u, t // 3, t % 3)).sum((0, 1, 2)) for t in range(9)]), dpre.sum((0, 1, 2))


def run_dw_bwd(u, dy, w9, bias, dtype, what, acc0=None):
    B, H, W, Cc = u.shape
    dpre = Framed((B, H, W, Cc), dtype)
    dw9 = Framed((9, Cc), F32, fill=None if acc0 is None else dev(acc0[0]))
    db = Framed((Cc,), F32, fill=None if acc0 is None else dev(acc0[1]))
    ws, nbytes = owned_ws(B * H * W, Cc, 10)
    ud, dyd, wd, bd = dev(u, dtype), dev(dy, dtype), dev(w9), dev(bias)
    LIB().gdl_dwconv3x3_gelu_bwd(P(ud), P(dyd), ops.dt(dtype), B, H, W, Cc, P(wd), P(bd),
                                 P(dpre.view), P(dw9.view), P(db.view), int(acc0 is not None), P(ws), nbytes, ops._stream())
    torch.cuda.synchronize()
    dpre.check(what + " dpre"), dw9.check(what + " dw9"), db.check(what + " db")
    return dpre.view, dw9.view, db.view, ws


def dw_bwd_exact(u, dy, dtype, what, acc0=None):
    """w9 = 0 and bias = 0: pre = 0, gelu'(0) = 0.5 by its formula, dpre = dy / 2 for even dy"""
    B, H, W, Cc = u.shape
    zero9, zero = torch.zeros(9, Cc, dtype=torch.float64), torch.zeros(Cc, dtype=torch.float64)
    dpre_ref = dy / 2
    dw_ref, db_ref = ref_dw_bwd(u, dpre_ref)
    dpre, dw9, db, ws = run_dw_bwd(u, dy, zero9, zero, dtype, what, acc0)
    same(dpre, dpre_ref, what + " dpre")
    same(dw9, dw_ref + (0 if acc0 is None else acc0[0]), what + " dw9")
    same(db, db_ref + (0 if acc0 is None else acc0[1]), what + " db")
    nblk, rb, items = dw_bwd_blocks(B, H, W, Cc)
    check_partials(ws, rb, 10 * Cc, items, nblk, torch.cat([dw_ref.reshape(-1), db_ref]), what)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=DT_ID.get)
@pytest.mark.parametrize("B,H,W,Cc", DWB_SHAPES)
def test_dwconv_gelu_bwd_exact(B, H, W, Cc, dtype):
    seed = 1000 * W + 10 * H + Cc
    u, dy = ints((B, H, W, Cc), seed, -3, 3), 2 * ints((B, H, W, Cc), seed + 1)
    dw_bwd_exact(u, dy, dtype, f"dwconv_gelu_bwd {DT_ID[dtype]} {B}x{H}x{W}x{Cc}")
    if (B, H, W, Cc) in DWB_SHAPES[:2]:
        acc0 = (ints((9, Cc), seed + 2, -100, 100), ints((Cc,), seed + 3, -100, 100))
        dw_bwd_exact(u, dy, dtype, f"dwconv_gelu_bwd accumulate {DT_ID[dtype]} {B}x{H}x{W}x{Cc}", acc0)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=DT_ID.get)
@pytest.mark.parametrize("B,H,W,Cc", DWB_BASIS)
def test_dwconv_gelu_bwd_basis(B, H, W, Cc, dtype):
    """dy one-hot and u dense: dw9[t] is the window that the walker showed at that pixel; then the reverse"""
    seed = 77 * W + Cc
    dense_u, dense_dy = ints((B, H, W, Cc), seed, -3, 3), 2 * ints((B, H, W, Cc), seed + 1)
    for y0, x0 in basis_pixels(H, W):
        hot = torch.zeros(B, H, W, Cc, dtype=torch.float64)
        hot[B - 1, y0, x0] = 2.0
        dw_bwd_exact(dense_u, hot, dtype, f"dwconv_gelu_bwd {DT_ID[dtype]} {B}x{H}x{W}x{Cc} dy one-hot at ({y0}, {x0})")
        dw_bwd_exact(hot / 2, dense_dy, dtype, f"dwconv_gelu_bwd {DT_ID[dtype]} {B}x{H}x{W}x{Cc} u one-hot at ({y0}, {x0})")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=DT_ID.get)
@pytest.mark.parametrize("B,H,W,Cc", [(2, 3, 33, 68), (1, 5, 70, 4), (2, 2, 35, 260)])
def test_dwconv_gelu_bwd_yardstick(B, H, W, Cc, dtype):
    """Random weights.  dpre = dy gelu'(pre): |gelu''| < 1, so an error of pre of the size of its terms moves dpre by at most
    |dy| times that; scale |dy| (1 + terms of pre).  The weight gradient is defined over dpre AS STORED (the kernel rounds it to
    the tensor's dtype first), so its reference and torch's f32 sum both run over the dpre that the kernel returned."""
    u, w9, bias, dy, s_pre = dw_real_operands(B, H, W, Cc, dtype)
    what = f"dwconv_gelu_bwd random {DT_ID[dtype]} {B}x{H}x{W}x{Cc}"

    def dpre_of(dt_):
        pre = ref_dwconv(u.to(dt_), w9.to(dt_), bias.to(dt_)).requires_grad_(True)
        F.gelu(pre).backward(dy.to(dt_))
        return pre.grad
    dpre, dw9, db, _ = run_dw_bwd(u, dy, w9, bias, dtype, what)
    check_yard(dpre, dpre_of(torch.float64), dpre_of(F32), dy.abs() * (1 + s_pre), dtype, what + " dpre")
    stored = dpre.double().cpu()
    dw_ref, db_ref = ref_dw_bwd(u, stored)
    dw_32, db_32 = ref_dw_bwd(u.float(), stored.float())
    s_dw, s_db = ref_dw_bwd(u.abs(), stored.abs())
    check_yard(dw9, dw_ref, dw_32, s_dw, F32, what + " dw9")
    check_yard(db, db_ref, db_32, s_db, F32, what + " db")


# ================================================================== 6. col2im
C2I_GEOS = [(7, 4, 3), (3, 2, 1), (2, 2, 0), (4, 4, 0), (8, 8, 0), (3, 1, 1), (1, 1, 0), (1, 2, 0)]       # (k, stride, pad)
C2I_HW = [(9, 7), (16, 16), (5, 70), (1, 1)]
C2I_C = (4, 32, 64)
C2I_LAYOUTS = ("dense", "channel slice", "row padded")


def c2i_cases():
    """(k, stride, pad, H, W, C, B) of every geometry whose kernel fits the padded map (otherwise there is no convolution)"""
    out = []
    for i, (k, st, pad) in enumerate(C2I_GEOS):
        for j, (H, W) in enumerate(C2I_HW):
            if conv_out(H, k, st, pad) >= 1 and conv_out(W, k, st, pad) >= 1:
                out.append((k, st, pad, H, W, C2I_C[(i + j) % 3], 1 + (i + j) % 2))
    return out


def ref_col2im(cols, B, Ho, Wo, k, Cc, stride, pad, H, W):
    """cols [B*Ho*Wo, (r, s, c)] float64 -> dx NHWC float64 through F.fold (whose channel order is (c, r, s))"""
    t = cols.view(B, Ho * Wo, k, k, Cc).permute(0, 4, 2, 3, 1).reshape(B, Cc * k * k, Ho * Wo)
    return F.fold(t, (H, W), (k, k), padding=pad, stride=stride).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("k,stride,pad,H,W,Cc,B", c2i_cases())
def test_col2im(k, stride, pad, H, W, Cc, B):
    Ho, Wo = conv_out(H, k, stride, pad), conv_out(W, k, stride, pad)
    cols = ints((B * Ho * Wo, k * k * Cc), 100 * k + 10 * H + W + Cc)
    ref = ref_col2im(cols, B, Ho, Wo, k, Cc, stride, pad, H, W)
    for in_dtype, out_dtype in PAIRS:
        cd = dev(cols, in_dtype)
        for layout in C2I_LAYOUTS:
            if layout == "dense":
                dx = Framed((B, H, W, Cc), out_dtype)
            elif layout == "channel slice":
                dx = Framed((B, H, W, Cc + 12), out_dtype, index=(Ellipsis, slice(4, 4 + Cc)))
            else:
                dx = Framed((B, H, W + 3, Cc), out_dtype, index=(slice(None), slice(None), slice(1, W + 1)))
            v = dx.view
            LIB().gdl_col2im(P(cd), ops.dt(in_dtype), B, Ho, Wo, k, k, Cc, stride, pad, H, W, P(v), ops.dt(out_dtype),
                             v.stride(0), v.stride(1), v.stride(2), ops._stream())
            torch.cuda.synchronize()
            what = f"col2im {DT_ID[in_dtype]}->{DT_ID[out_dtype]} k={k} s={stride} p={pad} {B}x{H}x{W}x{Cc} {layout}"
            same(v, ref, what)
            dx.check(what)


# ================================================================== 7. softmax backward (rows)
SMB_COLS = (1, 63, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048)
SMB_ROWS = (1, 5, 9)


def smb_valid(n_cols):
    return sorted({n_cols, max(1, n_cols - 1), max(1, n_cols - 37)})


def smb_case(rows, n_valid, n_cols, seed):
    """p: one-hot rows (even) or 1/2, 1/4, 1/4 on three seeded columns (odd, where there are three); dp integers; pad columns NaN"""
    gen = torch.Generator().manual_seed(seed)
    p = torch.zeros(rows, n_cols, dtype=torch.float64)
    for r in range(rows):
        idx = torch.randperm(n_valid, generator=gen)[:3]
        if r % 2 == 0 or n_valid < 3:
            p[r, idx[0]] = 1.0
        else:
            p[r, idx] = torch.tensor([0.5, 0.25, 0.25], dtype=torch.float64)
    dp = ints((rows, n_cols), seed + 1, -4, 4)
    scale = (0.125, 0.5, 1.0, 2.0)[seed % 4]
    ds = p * (dp - (p * dp).sum(1, keepdim=True)) * scale
    p[:, n_valid:], dp[:, n_valid:], ds[:, n_valid:] = NAN, NAN, 0.0
    return p, dp, ds, scale


@pytest.mark.parametrize("dtype", [F32, BF16], ids=DT_ID.get)
@pytest.mark.parametrize("n_cols", SMB_COLS)
def test_softmax_bwd_rows(n_cols, dtype):
    for rows in SMB_ROWS:
        for n_valid in smb_valid(n_cols):
            p, dp, ds_ref, scale = smb_case(rows, n_valid, n_cols, rows + n_valid + n_cols)
            for inplace in ((False, True) if rows == 5 else (False,)):
                what = f"softmax_bwd_rows {DT_ID[dtype]} rows={rows} n_valid={n_valid} n_cols={n_cols} inplace={inplace}"
                ds = Framed((rows, n_cols), dtype, fill=dev(dp, dtype) if inplace else None)
                pd, dpd = dev(p, dtype), ds.view if inplace else dev(dp, dtype)
                LIB().gdl_softmax_bwd_rows(P(pd), P(dpd), P(ds.view), ops.dt(dtype), rows, n_valid, n_cols, scale,
                                           ops._stream())
                torch.cuda.synchronize()
                same(ds.view, ds_ref, what)
                ds.check(what)


# ================================================================== 8. add_rows
# (rows, a_rows, b_rows or None, D)
ADD_ROWS = [(7, 7, 7, 5), (12, 3, 4, 33), (10, 1, 10, 64), (9, 4, None, 130), (600, 7, 52, 260), (5, 5, 2, 1)]


@pytest.mark.parametrize("rows,a_rows,b_rows,D", ADD_ROWS)
def test_add_rows(rows, a_rows, b_rows, D):
    gen = torch.Generator().manual_seed(rows + D)
    for strided in (False, True):
        pad = 3 if strided else 0
        a = torch.randn(a_rows, D + pad, generator=gen)[:, pad:]
        b = None if b_rows is None else torch.randn(b_rows, D + 2 * pad, generator=gen)[:, pad:pad + D]
        r = torch.arange(rows)
        ref = a[r % a_rows] + (0 if b is None else b[r % b_rows])            # the CPU's f32 sum: one rounding, the same bits
        ad = a.to(DEV) if not strided else torch.randn(a_rows, D + pad, device=DEV)[:, pad:].copy_(a)
        bd = None if b is None else (b.to(DEV) if not strided else torch.randn(b_rows, D + 2 * pad, device=DEV)[:, pad:pad + D].copy_(b))
        out = Framed((rows, D + 2 * pad), F32, index=(slice(None), slice(pad, pad + D)))
        assert ad.stride(0) == D + pad and out.view.stride(0) == D + 2 * pad
        ops.add_rows(ad, bd, out.view, rows)
        torch.cuda.synchronize()
        what = f"add_rows rows={rows} a_rows={a_rows} b_rows={b_rows} D={D} strided={strided}"
        assert torch.equal(out.view.cpu(), ref), what
        out.check(what)
