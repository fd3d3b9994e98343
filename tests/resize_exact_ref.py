"""Exact references, exactness proofs and case tables of the resized-conv gather kernels (csrc/resize_conv_fwd.hip, csrc/resize_conv_bwd.hip), shared by
test_resize_exact_host.py (CPU: proves every case exact) and test_hip_resize_exact.py (GPU: compares bits).  float64 on the CPU.

For resize factors f = 2, 4, 8 the bilinear weights (align_corners=False, edges clamped) are k / (2 f); the weight of a tap is
a product of two of them, a multiple of the quantum q = 1 / (2 f)^2, and exact in bf16 (numerators below 2^8).  With integer
operands every product and every partial sum is a multiple of q; while sum|terms| / q stays below 2^24 every such sum is an f32
value, in any order and in any MFMA accumulator, so the f32 result is THE sum, and the one bf16 store (round to nearest even)
leaves exactly one correct bit pattern.  ``assert_exact`` proves the premises per case; nothing here or in the GPU file has a
tolerance, except for the BatchNorm variance (E[x^2] - m^2 from f32 partial sums of squares), which is not claimed exact.
"""

import functools

import torch

EXACT = float(1 << 24)
F32, BF16 = 0, 1                      # GDL_F32 / GDL_BF16


# ------------------------------------------------------------------ operands
def ints(shape, seed, lo=-2, hi=2):
    """Seeded integer-valued CPU tensor (float64) with lo <= v <= hi."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g).double()
    assert t.numel() == 0 or (t.min().item() >= lo and t.max().item() <= hi)
    return t


# ------------------------------------------------------------------ the operator
@functools.lru_cache(maxsize=None)
def interp_matrix(h, f):
    """[f h, h] float64: row o holds the bilinear weights of output position o (F.interpolate, align_corners=False)."""
    u = torch.zeros(f * h, h, dtype=torch.float64)
    for o in range(f * h):
        src = max((o + 0.5) / f - 0.5, 0.0)
        y0 = min(int(src), h - 1)
        y1 = min(y0 + 1, h - 1)
        l = src - y0
        u[o, y0] += 1.0 - l
        u[o, y1] += l
    k = u * (2 * f)
    assert torch.equal(k, k.round()), "bilinear weights of an integer factor are k / (2 f)"
    assert torch.equal(u.sum(1), torch.ones(f * h, dtype=torch.float64))
    return u


def shifted(u, d):
    """Rows of u moved so that row o holds u[o + d]; positions outside the output are zero (the convolution's padding)."""
    out = torch.zeros_like(u)
    n = u.shape[0]
    lo, hi = max(0, -d), min(n, n - d)
    if hi > lo:
        out[lo:hi] = u[lo + d:hi + d]
    return out


def _factor(h, H):
    f = H // h
    assert f in (2, 4, 8) and f * h == H, (h, H)
    return f


def fwd_sum_ref(zs, size):
    """out[b,oy,ox,n] = sum_k sum_(r,s) sum_(y,x) Uy[oy+r-1,y] Ux[ox+s-1,x] z_k[b,y,x,(3r+s) N + n];  zs: [B,h_k,w_k,9N] float64."""
    H, W = size
    B, N = zs[0].shape[0], zs[0].shape[3] // 9
    out = torch.zeros(B, H, W, N, dtype=torch.float64)
    for z in zs:
        assert z.dtype == torch.float64
        uy, ux = interp_matrix(z.shape[1], _factor(z.shape[1], H)), interp_matrix(z.shape[2], _factor(z.shape[2], W))
        for r in range(3):
            rows = torch.einsum("oy,byxm->boxm", shifted(uy, r - 1), z[..., 3 * r * N:(3 * r + 3) * N])      # the three taps of row r
            for s in range(3):
                out += torch.einsum("px,boxn->bopn", shifted(ux, s - 1), rows[..., s * N:(s + 1) * N])
    return out


def bwd_rows_ref(dy, Hi):
    """The two-pass gather's intermediate R_r[b,iy,ox,n] = sum_oy Uy[oy+r-1,iy] dy[b,oy,ox,n] as [3][B,Hi,Wo,N]."""
    uy = interp_matrix(Hi, _factor(Hi, dy.shape[1]))
    return torch.stack([torch.einsum("oy,boxn->byxn", shifted(uy, r - 1), dy) for r in range(3)])


def bwd_gather_ref(dy, in_size):
    """The transpose of fwd_sum_ref: g[b,y,x,(8-t) N + n] = sum_(oy,ox) Uy[oy+r-1,y] Ux[ox+s-1,x] dy[b,oy,ox,n], t = 3r+s."""
    Hi, Wi = in_size
    B, Ho, Wo, N = dy.shape
    assert dy.dtype == torch.float64
    ux = interp_matrix(Wi, _factor(Wi, Wo))
    rows = bwd_rows_ref(dy, Hi)
    g = torch.empty(B, Hi, Wi, 9 * N, dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            t = 3 * r + s
            g[..., (8 - t) * N:(9 - t) * N] = torch.einsum("px,bypn->byxn", shifted(ux, s - 1), rows[r])
    return g


def bn_dy_ref(dz, x, a, thr, c2, c3):
    """a (x a > thr ? dz : 0) - (c2 x + c3) per channel: the documented formula of bn_bwd_coef_kernel / the BN-fused gather."""
    return a * torch.where(x * a > thr, dz, torch.zeros_like(dz)) - (c2 * x + c3)


def bn_coefs(gamma, beta, relu, k1, k2):
    """(a, thr, c2, c3) for mean 0, var 1, eps 0 (rstd = 1): a = gamma, thr = -beta (-inf without ReLU), c2 = a k2, c3 = a k1."""
    a = gamma.double()
    thr = -beta.double() if relu else torch.full_like(a, -float("inf"))
    return a, thr, a * k2.double(), a * k1.double()


# ------------------------------------------------------------------ proofs and comparisons
def is_bf16(x64):
    return torch.equal(x64.bfloat16().double(), x64)


def assert_exact(operands, q, abs_sums, stored=(), unit=1.0, what=""):
    """The premises of a bit-exact comparison.  ``operands``: the float64 inputs, integers (times ``unit``, a power of two, when
    they are themselves a stored intermediate); ``q``: the weight quantum 1 / (2 f)^2 of the case; ``abs_sums``: the operator
    with absolute values applied to |operands| (+ |addend|), one tensor per accumulation -- its largest element over q * unit is
    the largest numerator any partial sum can reach and must stay below 2^24; ``stored``: everything a kernel rounds to bf16
    before the final result, which must be bf16 values already.  Returns the largest numerator."""
    for t in operands:
        assert torch.equal(t / unit, (t / unit).round()), f"{what}: operands must be integers"
        assert is_bf16(t), f"{what}: operands must be bf16 values"
    worst = max(float(s.max()) for s in abs_sums) / (q * unit)
    assert worst < EXACT, f"{what}: partial sums reach {worst} quanta >= 2^24: not exact in f32"
    for t in stored:
        assert is_bf16(t), f"{what}: an intermediate the kernel stores in bf16 is not a bf16 value"
    return worst


def to_bf16_rne(x64):
    """float64 -> f32 (exact under assert_exact's bound) -> bf16, one round-to-nearest-even step."""
    f = x64.float()
    assert torch.equal(f.double(), x64), "the reference is not an f32 value"
    return f.bfloat16()


def expected(ref64, dtype):
    return to_bf16_rne(ref64) if dtype == torch.bfloat16 else ref64.float()


def assert_same(got, ref, what):
    """torch.equal with a message that says how the result differs."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if torch.equal(got, ref.to(got.device)):
        return
    got, ref = got.detach().cpu().float(), ref.detach().cpu().float()
    bad = (got != ref) | got.isnan()
    first = bad.nonzero()[0].tolist()
    diff = (got - ref)[bad & ~got.isnan()].abs()
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(got.isnan().sum())} NaN, largest "
                         f"finite difference {diff.max().item() if diff.numel() else 0.0}), first at {first}: "
                         f"got {got[tuple(first)].item()} want {ref[tuple(first)].item()}")


# ------------------------------------------------------------------ the forward's planner (csrc/resize_conv_fwd.hip: tapsum_plan)
VALU, V1, V2, ROLL, ROLL3 = range(5)
CUS = 256                             # the MI355X's; the `walks` digit of every code below counts on it


def code(kind, p, q, walks=0):
    """gdl_resize_conv3x3_fwd_sum_plan's code (include/gdlhip.h)."""
    return 1000 * kind + 100 * p + 10 * q + walks


def window_bytes(cols, lf):
    win = 4 if lf == 1 else 3
    return (win * (((cols - 4) >> lf) + win) * 9 * 128 + 1023) // 1024 * 1024


def plan_mirror(factors, dtype, B, N, Ho, Wo, stats=False, mfma=1, vec=0, roll=1, persist=1, cus=CUS):
    """What tapsum_plan decides for 16-byte aligned pointers, written out again from its rules: the host test holds the
    library's query to it at every designed shape, the GPU test asserts the query before it launches."""
    lfs = [{2: 1, 4: 2, 8: 3}[f] for f in factors]
    nsrc, run = len(factors), max(max(factors), 2)
    assert Wo % run == 0
    mfma_ok = dtype == BF16 and N % 64 == 0 and B * ((Ho + 3) // 4) <= 65535
    assert mfma_ok or not stats
    if mfma_ok and (mfma or stats):
        nstrips, ncols = (Wo + 15) // 16, B * (N // 64)
        if roll and not stats and lfs == [1, 2, 3] and Ho % 8 == 0 and mfma == 1:
            streams = max(min(cus // nstrips, ncols), 1)
            return code(ROLL3, 3, 2, int(ncols > streams))
        if roll and nsrc == 1 and lfs[0] in (1, 2) and Ho % 4 == 0 and Ho >= 8 and (mfma == 1 or stats):
            G = max(min((cus // 8 * (3 if lfs[0] == 2 else 2)) // nstrips, (ncols + 7) // 8), 1)
            return code(ROLL, lfs[0], (1 if roll == 2 else 3) if lfs[0] == 2 else 1, int(ncols > 8 * G))
        if (mfma == 1 and nsrc == 1 and lfs[0] >= 2) or mfma == 5 or stats:
            ring = sum(window_bytes(16, lfs[0 if nsrc == 1 else j]) for j in range(2 if nsrc == 1 else nsrc))
            assert nsrc * (256 + 16 * 64) + 4 * 16 * 128 + ring <= 160 * 1024
            nblk = ((Wo + 15) // 16) * B * ((Ho + 3) // 4)
            return code(V2, nsrc, lfs[0] if nsrc == 1 else 0, int(bool(persist) and nblk > cus * (3 if nsrc == 1 else 1)))
        return code(V1, 2 if window_bytes(32, min(lfs)) <= 48 * 1024 and mfma != 4 else 1, 0)
    v = 8 if dtype == BF16 else 4
    if dtype == BF16 and (vec == 4 or N % 8 != 0 or (run == 8 and vec != 8)):
        v = 4
    return code(VALU, v, run)


# every form of the forward: name -> (operand dtype, hooks).  Hooks: gdl_debug_set_tapsum_mfma / _vec / _roll / _persist.
FORMS = {
    "valu-f32": (torch.float32, dict()),
    "valu-bf16-16B": (torch.bfloat16, dict(mfma=0, vec=8)),
    "valu-bf16-8B": (torch.bfloat16, dict(mfma=0, vec=4)),
    "v1-16col": (torch.bfloat16, dict(mfma=4)),
    "v1-32col": (torch.bfloat16, dict(mfma=2)),
    "v2": (torch.bfloat16, dict(mfma=5)),
    "v2-one-patch-per-workgroup": (torch.bfloat16, dict(mfma=5, persist=0)),
    "production": (torch.bfloat16, dict()),
    "production-no-roll": (torch.bfloat16, dict(roll=0)),
}


def form_code(name, B, H, W, N, factors):
    dtype, hooks = FORMS[name]
    return plan_mirror(factors, BF16 if dtype == torch.bfloat16 else F32, B, N, H, W, **hooks)


def forms_of(B, H, W, N, factors):
    """{form name: plan code} of the DISTINCT kernel forms this shape admits: the production choice first, then each forced
    form whose code differs from the ones before it (a hook that changes nothing for this shape adds no case)."""
    out, seen = {}, set()
    for name in ["production", "production-no-roll", "v2", "v2-one-patch-per-workgroup", "v1-32col", "v1-16col", "valu-bf16-16B",
                 "valu-bf16-8B", "valu-f32"]:
        if FORMS[name][0] == torch.bfloat16 and N % 8 and name != "production":
            continue                                  # (N % 8 != 0: the 8-byte pixel kernel is the only bf16 form)
        c = (FORMS[name][0], form_code(name, B, H, W, N, factors))
        if c not in seen:
            seen.add(c)
            out[name] = c[1]
    return out


# ------------------------------------------------------------------ case tables
# a. forward basis: (factor, (h, w)) onto 8 x 16, N = 64, one impulse per (b, n)
BASIS_OUT, BASIS_N = (8, 16), 64
FWD_BASIS = {2: (4, 8), 4: (2, 4), 8: (1, 2)}

# b. forward dense: id -> ((B, H, W, N, factors), hooks of the designed form, its code on an MI355X, what it exercises)
FWD_DENSE = {
    "strips-2full-1partial": ((2, 8, 40, 64, (2,)), {}, code(ROLL, 1, 1), "two full 16-column strips and a partial one"),
    "x4-two-chunks": ((2, 12, 40, 128, (4,)), {}, code(ROLL, 2, 3), "Ho % 4 == 0, two channel chunks"),
    "ragged-row-block": ((1, 6, 24, 64, (2,)), {}, code(V1, 1, 0), "Ho % 4 != 0: versions 1 / 2, a ragged last row block"),
    "x8-version2": ((1, 16, 16, 64, (8,)), {}, code(V2, 1, 3), "version 2 with LF = 3"),
    "two-sources": ((2, 16, 32, 64, (8, 4)), {}, code(V1, 2, 0), "two sources"),
    "roll3-one-cell": ((1, 8, 16, 64, (2, 4, 8)), {}, code(ROLL3, 3, 2), "one cell of the coarsest level"),
    "roll3-steps-strips": ((3, 24, 40, 128, (2, 4, 8)), {}, code(ROLL3, 3, 2), "roll3 over several steps and strips"),
    "n72-valu": ((1, 8, 16, 72, (4, 2)), {}, code(VALU, 8, 4), "N % 64 != 0: the pixel kernel in bf16"),
    "n68-valu-8B": ((1, 8, 16, 68, (2, 4)), {}, code(VALU, 4, 4), "N % 8 != 0: the pixel kernel falls back to 8-byte bf16 vectors"),
    # the next two count on 256 CUs: 1024 patches against 3 * 256 resident workgroups; 260 columns against 8 * 32 column groups
    "v2-persistent-second-patch": ((4, 64, 256, 64, (4,)), dict(roll=0), code(V2, 1, 2, 1), "the persistent version-2 walk takes a second patch"),
    "roll-second-column": ((65, 32, 40, 256, (4,)), {}, code(ROLL, 2, 3, 1), "a rolling-window workgroup walks a second, pre-primed column"),
}

# c. forward with statistics: (B, H, W, N), factor 2; operands in -1..1 so that every output is a bf16 value before rounding
FWD_STATS = [(1, 8, 16, 64), (2, 16, 24, 64)]

# d. backward basis: dy 8 x 16, B = 2, N = 64; (factor, (Hi, Wi)), and the two extra maps at factor 4
BWD_BASIS = [(2, (4, 8)), (4, (2, 4)), (8, (1, 2))]
BWD_BASIS_EXTRA = [(4, (1, 1)), (4, (2, 13))]

# e. backward dense (B, Hi, Wi, N, f)
BWD_DENSE = [(2, 5, 7, 64, 4), (2, 9, 6, 128, 2), (1, 3, 4, 128, 8), (1, 2, 13, 128, 4), (2, 1, 1, 64, 4), (1, 6, 10, 192, 2)]

# f. BatchNorm-backward-fused gather
BN_SHAPES = [(2, 5, 7, 64, 4), (2, 9, 6, 128, 2), (1, 2, 13, 128, 4)]
BN_CASES = ["i", "ii", "iii", "iv"]

# g. plain resamplers (hi, wi, f, C)
RESAMPLE = [(2, 2, 4, 8), (7, 5, 4, 72), (9, 13, 2, 64)]


def gather_forms(dtype, f):
    """The backward gather's forms for (dtype, factor): (name, gdl_debug_set_gather_mfma, ops.GATHER_TWO_PASS)."""
    forms = [("two-pass", 0, True), ("single-pass", 0, False)]
    if dtype == torch.bfloat16 and f in (2, 4):
        forms.insert(0, ("one-pass-mfma", 1, True))
    return forms


# ------------------------------------------------------------------ problems (computed once, shared, never modified)
@functools.lru_cache(maxsize=None)
def fwd_basis_problem(f):
    """(z, reference) of the exhaustive basis: element (b, n) carries a unit impulse at source index (pixel, tap) = b N + n."""
    h, w = FWD_BASIS[f]
    N, total = BASIS_N, h * w * 9
    B = -(-total // N)
    z = torch.zeros(B, h, w, 9 * N, dtype=torch.float64)
    for i in range(total):
        b, n, (pix, tap) = i // N, i % N, divmod(i, 9)
        z[b, pix // w, pix % w, tap * N + n] = 1.0
    ref = fwd_sum_ref([z], BASIS_OUT)
    assert_exact([z], 1.0 / (2 * f) ** 2, [ref.abs()], what=f"forward basis x{f}")
    assert is_bf16(ref), "a single weight product is a bf16 value"
    return z, ref


@functools.lru_cache(maxsize=None)
def fwd_dense_problem(name, lo=-2, hi=2):
    """(zs, addvec, reference, reference with addvec + ReLU) of one dense forward case."""
    (B, H, W, N, factors), _, _, _ = FWD_DENSE[name] if isinstance(name, str) else (name, None, None, None)
    zs = [ints((B, H // f, W // f, 9 * N), 100 + 7 * f + H, lo, hi) for f in factors]
    add = ints((N,), 5 + H, -3, 3)
    ref = fwd_sum_ref(zs, (H, W))
    absref = fwd_sum_ref([z.abs() for z in zs], (H, W)) + add.abs()
    assert_exact(zs + [add], 1.0 / (2 * max(factors)) ** 2, [absref], what=f"forward {name}")
    return zs, add, ref, torch.relu(ref + add)


@functools.lru_cache(maxsize=None)
def bwd_basis_problem(f, in_size):
    """(dy, reference): one unit impulse per (b, n) over the 128 output pixels of an 8 x 16 map -- or of f * in_size."""
    Ho, Wo = f * in_size[0], f * in_size[1]
    N = BASIS_N
    B = -(-Ho * Wo // N)
    dy = torch.zeros(B, Ho, Wo, N, dtype=torch.float64)
    for p in range(Ho * Wo):
        dy[p // N, p // Wo, p % Wo, p % N] = 1.0
    ref = bwd_gather_ref(dy, in_size)
    rows = bwd_rows_ref(dy, in_size[0])
    assert_exact([dy], 1.0 / (2 * f) ** 2, [ref.abs()], stored=[rows], what=f"backward basis x{f} {in_size}")
    assert is_bf16(ref)
    return dy, ref


@functools.lru_cache(maxsize=None)
def bwd_dense_problem(B, Hi, Wi, N, f):
    """(dy in -1..1, reference); the two-pass form's bf16 rows workspace is proven exact."""
    dy = ints((B, f * Hi, f * Wi, N), 300 + Hi * Wi + f, -1, 1)
    ref = bwd_gather_ref(dy, (Hi, Wi))
    assert_exact([dy], 1.0 / (2 * f) ** 2, [bwd_gather_ref(dy.abs(), (Hi, Wi))], stored=[bwd_rows_ref(dy, Hi)],
                 what=f"backward dense {(B, Hi, Wi, N, f)}")
    return dy, ref


@functools.lru_cache(maxsize=None)
def bn_problem(case, shape, relu):
    """One BatchNorm-backward-fused case: dict of the float64 operands, the per-channel constants as the op takes them, the
    transformed gradient and the gathered reference.  mean 0, var 1, eps 0 throughout."""
    B, Hi, Wi, N, f = shape
    Ho, Wo = f * Hi, f * Wi
    P = B * Ho * Wo
    seed = 400 + Hi * Wi + f
    dz = ints((B, Ho, Wo, N), seed, -1, 1)
    ch = torch.arange(N)
    if case == "iv":
        assert relu
        gamma, beta = torch.ones(N, dtype=torch.float64), torch.ones(N, dtype=torch.float64)
        x = ints((B, Ho, Wo, N), seed + 1, -2, 2)
        assert (x == -1).any()                                    # elements exactly on the threshold thr = -1
    else:
        gamma, beta = torch.tensor([1.0, 2.0, -1.0], dtype=torch.float64)[ch % 3], torch.zeros(N, dtype=torch.float64)
        x = ints((B, Ho, Wo, N), seed + 1, -1, 1)
    k1 = torch.tensor([0.0, 1.0, -1.0], dtype=torch.float64)[(ch // 3) % 3] if case == "ii" else torch.zeros(N, dtype=torch.float64)
    k2 = torch.tensor([0.0, 0.5, -0.5], dtype=torch.float64)[(ch // 3) % 3] if case == "iii" else torch.zeros(N, dtype=torch.float64)
    a, thr, c2, c3 = bn_coefs(gamma, beta, relu, k1, k2)
    dy = bn_dy_ref(dz, x, a, thr, c2, c3)
    ref = bwd_gather_ref(dy, (Hi, Wi))
    sums = (P * k2).float(), (P * k1).float()                      # dgamma_sum, dbeta_sum
    assert torch.equal(sums[0].double(), P * k2) and torch.equal(sums[1].double(), P * k1)
    assert_exact([dz, x], 1.0, [dz.abs()], what=f"bn {case} operands")
    assert_exact([dy], 1.0 / (2 * f) ** 2, [bwd_gather_ref(dy.abs(), (Hi, Wi))], stored=[dy, bwd_rows_ref(dy, Hi)], unit=0.5,
                 what=f"bn {case} {shape} relu={relu}")
    return dict(dz=dz, x=x, gamma=gamma, beta=beta, dgamma_sum=sums[0], dbeta_sum=sums[1], P=P, dy=dy, ref=ref, coefs=(a, thr, c2, c3))


def resize_ref(x, f):
    """interp_matrix on both sides of x [B,h,w,C] float64."""
    uy, ux = interp_matrix(x.shape[1], f), interp_matrix(x.shape[2], f)
    return torch.einsum("oy,px,byxc->bopc", uy, ux, x)


def resize_t_ref(dy, f):
    """The transpose of resize_ref: dy [B,f h,f w,C] -> [B,h,w,C]."""
    uy, ux = interp_matrix(dy.shape[1] // f, f), interp_matrix(dy.shape[2] // f, f)
    return torch.einsum("oy,px,bopc->byxc", uy, ux, dy)


@functools.lru_cache(maxsize=None)
def resample_problem(hi, wi, f, C):
    """(x, resized reference, dout, transposed reference) of a plain integer-factor resampler case, B = 2."""
    x, dout = ints((2, hi, wi, C), 500 + hi), ints((2, f * hi, f * wi, C), 501 + hi)
    up, down = resize_ref(x, f), resize_t_ref(dout, f)
    q = 1.0 / (2 * f) ** 2
    assert_exact([x], q, [resize_ref(x.abs(), f)], what="resize")
    assert_exact([dout], q, [resize_t_ref(dout.abs(), f)], what="resize transpose")
    return x, up, dout, down


@functools.lru_cache(maxsize=None)
def node_problem(f=4):
    """conv3x3(pad 1)(bilinear x f (x)) with x, w in -1..1, C = N = 64 on a 4 x 6 map, B = 2: forward, and dw / dx_lo from a
    gradient dy in -1..1 through the nine gathered maps G, which the kernels store in bf16 -- so does the reference."""
    B, h, w_, Cc, N = 2, 4, 6, 64, 64
    H, W = f * h, f * w_
    q = 1.0 / (2 * f) ** 2
    x, wt, dy = ints((B, h, w_, Cc), 601, -1, 1), ints((N, Cc, 3, 3), 602, -1, 1), ints((B, H, W, N), 603, -1, 1)
    taps = wt.permute(2, 3, 0, 1).reshape(9 * N, Cc)                       # row t N + n
    z = torch.einsum("byxc,mc->byxm", x, taps)                             # |z| <= 64: bf16 integers
    y = fwd_sum_ref([z], (H, W))
    assert_exact([x, wt], 1.0, [torch.einsum("byxc,mc->byxm", x.abs(), taps.abs())], stored=[z], what="node tap products")
    assert_exact([z], q, [fwd_sum_ref([z.abs()], (H, W))], what="node forward")
    g = bwd_gather_ref(dy, (h, w_))
    assert_exact([dy], q, [bwd_gather_ref(dy.abs(), (h, w_))], stored=[bwd_rows_ref(dy, h)], what="node gather")
    gb = to_bf16_rne(g).double()                                           # G as the kernels store it
    wflip = wt.permute(2, 3, 0, 1).flip(0, 1).reshape(9 * N, Cc)           # row (8 - t) N + n: G's tap order
    dx = torch.einsum("byxm,mc->byxc", gb, wflip)
    dwp = torch.einsum("byxm,byxc->mc", gb, x)                             # [(8 - t, n), c]
    dw = dwp.view(9, N, Cc).flip(0).permute(1, 0, 2).reshape(N, 3, 3, Cc).permute(0, 3, 1, 2)
    # G (bf16) keeps the quantum q; its products with integers in -1..1 sum over 9 N channels (dx) or B h w pixels (dw)
    assert torch.equal(gb / q, (gb / q).round())
    assert_exact([], q, [torch.einsum("byxm,mc->byxc", gb.abs(), wflip.abs()), torch.einsum("byxm,byxc->mc", gb.abs(), x.abs())],
                 stored=[gb], what="node gradients")
    # the statistics the forward emits are those of the STORED (bf16) outputs: they keep the quantum q, their per-channel sum is exact
    yb = to_bf16_rne(y).double().reshape(-1, N)
    assert torch.equal(yb / q, (yb / q).round()) and yb.abs().sum(0).max().item() / q < EXACT
    return dict(x=x, w=wt, dy=dy, y=y, dx=dx, dw=dw.contiguous(), size=(H, W), mean=yb.mean(0), var=yb.var(0, unbiased=False))
