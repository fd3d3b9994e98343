"""Exact tests of the resized-conv gather kernels (csrc/resize_conv_fwd.hip, csrc/resize_conv_bwd.hip; the plain resamplers: csrc/resample.hip): the forward gdl_resize_conv3x3_fwd_sum in every form
(pixel-by-pixel kernel, matrix-core versions 1 and 2, rolling window, roll3), with BatchNorm statistics, and the backward
gdl_resize_conv3x3_bwd_gather in every form (one-pass matrix cores, two-pass rows / columns, single pass, BatchNorm backward
fused), plus the plain integer-factor resamplers and one conv3x3(resize(x)) node end to end.

Operands are small integers and the resize factors 2, 4, 8, so every weight is a dyadic rational that bf16 holds, every partial
sum is an f32 value in any order, and each output has exactly one correct bit pattern (tests/resize_exact_ref.py says why and
test_resize_exact_host.py proves it for every case table on the CPU).  Every comparison here is ``torch.equal`` against that
pattern (the BatchNorm variance alone, a difference of f32 sums of squares, is held to the suite's f32 tolerance): a dropped or doubled border contribution, a tap attributed to the neighbouring cell, a stale ring row are hard
failures at whatever scale they occur.  Outputs and workspaces the test can own are pre-filled with NaN.  Every forward case
asserts the kernel form it was designed for (gdl_resize_conv3x3_fwd_sum_plan) and fails loudly when a change of the launcher
moves its shape to another form; the codes whose last digit depends on the CU count are those of an MI355X (256 CUs).
"""

import contextlib
import ctypes as C

import pytest
import torch

import resize_exact_ref as R

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import _lib, nn as gnn, ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")
DT = {torch.float32: R.F32, torch.bfloat16: R.BF16}


# ------------------------------------------------------------------ hooks and launchers
@contextlib.contextmanager
def hooks(mfma=1, vec=0, roll=1, persist=1, gather_mfma=1, two_pass=True):
    """Kernel selection through the existing gdl_debug_* hooks and ops.GATHER_TWO_PASS; always reset."""
    lib = _lib.load()

    def put(m, v, r, p, g, t):
        lib.gdl_debug_set_tapsum_mfma(m), lib.gdl_debug_set_tapsum_vec(v), lib.gdl_debug_set_tapsum_roll(r)
        lib.gdl_debug_set_tapsum_persist(p), lib.gdl_debug_set_gather_mfma(g)
        ops.GATHER_TWO_PASS = t
    put(mfma, vec, roll, persist, gather_mfma, two_pass)
    try:
        yield
    finally:
        put(1, 0, 1, 1, 1, True)


def nans(shape, dtype):
    return torch.full(tuple(shape), NAN, device=DEV, dtype=dtype)


def sources(zs):
    n = len(zs)
    return ((C.c_void_p * 3)(*([z.data_ptr() for z in zs] + [None] * (3 - n))), (C.c_int * 3)(*([z.shape[1] for z in zs] + [1] * (3 - n))),
            (C.c_int * 3)(*([z.shape[2] for z in zs] + [1] * (3 - n))), n)


def plan(zs, size, stats=False):
    _, hs, ws, n = sources(zs)
    B, N = zs[0].shape[0], zs[0].shape[3] // 9
    return _lib.load().gdl_resize_conv3x3_fwd_sum_plan(hs, ws, n, DT[zs[0].dtype], B, N, size[0], size[1], int(stats))


def fwd_sum(zs, size, addvec=None, relu=False):
    """gdl_resize_conv3x3_fwd_sum as ops.resize_conv3x3_fwd_sum calls it, into a NaN-filled output."""
    ptrs, hs, ws, n = sources(zs)
    B, N = zs[0].shape[0], zs[0].shape[3] // 9
    out = nans((B, size[0], size[1], N), zs[0].dtype)
    _lib.checked().gdl_resize_conv3x3_fwd_sum(ptrs, hs, ws, n, DT[zs[0].dtype], B, N, out.data_ptr(), size[0], size[1],
                                              None if addvec is None else addvec.data_ptr(), int(relu), ops._stream())
    return out


def fwd_sum_bn(zs, size, addvec):
    """gdl_resize_conv3x3_fwd_sum_bn into NaN-filled output, statistics and workspace."""
    ptrs, hs, ws, n = sources(zs)
    B, N = zs[0].shape[0], zs[0].shape[3] // 9
    lib = _lib.checked()
    out, mean, var = nans((B, size[0], size[1], N), zs[0].dtype), nans((N,), torch.float32), nans((N,), torch.float32)
    wsp = nans((lib.gdl_resize_conv3x3_fwd_sum_bn_rows(B, size[0], size[1]) * 2 * N,), torch.float32)
    lib.gdl_resize_conv3x3_fwd_sum_bn(ptrs, hs, ws, n, DT[zs[0].dtype], B, N, out.data_ptr(), size[0], size[1], addvec.data_ptr(),
                                      wsp.data_ptr(), wsp.numel() * 4, mean.data_ptr(), var.data_ptr(), None, None, 0.1, ops._stream())
    return out, mean, var


def gather(dyd, in_size, form):
    """One form of the backward gather into a NaN-filled g (and, two-pass, a NaN-filled workspace of exactly the size the
    query asks for); then the same form through ops.resize_conv3x3_bwd_gather, which must give the same bits."""
    name, mfma, two_pass = form
    B, Ho, Wo, N = dyd.shape
    Hi, Wi = in_size
    lib = _lib.checked()
    g = nans((B, Hi, Wi, 9 * N), dyd.dtype)
    with hooks(gather_mfma=mfma, two_pass=two_pass):
        one_pass = lib.gdl_resize_conv3x3_bwd_gather_one_pass(DT[dyd.dtype], B, Ho, Wo, N, Hi, Wi)
        assert one_pass == int(name == "one-pass-mfma"), f"{name}: gdl_resize_conv3x3_bwd_gather_one_pass says {one_pass}"
        if name == "two-pass":
            nbytes = lib.gdl_resize_conv3x3_bwd_gather_workspace(DT[dyd.dtype], B, Wo, N, Hi)
            assert nbytes == 3 * B * Hi * Wo * N * dyd.element_size()
            ws = nans((nbytes // dyd.element_size(),), dyd.dtype)
            lib.gdl_resize_conv3x3_bwd_gather2(dyd.data_ptr(), DT[dyd.dtype], B, Ho, Wo, N, g.data_ptr(), Hi, Wi, ws.data_ptr(), nbytes,
                                               ops._stream())
        else:
            lib.gdl_resize_conv3x3_bwd_gather(dyd.data_ptr(), DT[dyd.dtype], B, Ho, Wo, N, g.data_ptr(), Hi, Wi, ops._stream())
        g_ops = ops.resize_conv3x3_bwd_gather(dyd, in_size)
    assert torch.equal(g_ops, g) or g.isnan().any(), f"{name}: ops.resize_conv3x3_bwd_gather differs from the direct call"
    return g


def check_forward_forms(B, H, W, N, factors, zs, cases, what, designed=None):
    """Every form the shape admits, forced in turn, asserted by its plan code, bit-identical to the one reference.
    cases: [(addvec or None, relu, float64 reference)]."""
    forms = R.forms_of(B, H, W, N, factors)
    if designed is not None:
        hk, want = designed
        with hooks(**hk):
            got = plan([z.to(DEV, torch.bfloat16) for z in zs], (H, W))
        assert got == want, f"{what}: designed for form {want}, the launcher plans {got}"
        assert want in forms.values()
    dev = {}
    for name, want in forms.items():
        dtype, hk = R.FORMS[name]
        if dtype not in dev:
            dev[dtype] = ([z.to(DEV, dtype) for z in zs], [None if a is None else a.float().to(DEV) for a, _, _ in cases],
                          [R.expected(ref, dtype).to(DEV) for _, _, ref in cases])
        zd, adds, refs = dev[dtype]
        with hooks(**hk):
            got = plan(zd, (H, W))
            assert got == want, f"{what} {name}: form {want} expected, the launcher plans {got}"
            outs = [fwd_sum(zd, (H, W), a, relu) for a, (_, relu, _) in zip(adds, cases)]
        torch.cuda.synchronize()
        for out, ref, (a, relu, _) in zip(outs, refs, cases):
            R.assert_same(out, ref, f"{what} form {name} (code {want}){' + addvec + ReLU' if relu else ''}")
    return forms


# ------------------------------------------------------------------ a. forward, exhaustive basis
@pytest.mark.parametrize("f", list(R.FWD_BASIS))
def test_forward_basis_every_form(f):
    """One unit impulse per (batch, channel) at every (source pixel, tap): each output channel is one column of the operator,
    a single weight product that bf16 holds -- the complete linear map at this shape, and a channel permutation shows."""
    z, ref = R.fwd_basis_problem(f)
    H, W = R.BASIS_OUT
    forms = check_forward_forms(z.shape[0], H, W, R.BASIS_N, (f,), [z], [(None, False, ref)], f"forward basis x{f}")
    kinds = {c // 1000 for c in forms.values()}
    assert {R.VALU, R.V1, R.V2} <= kinds and ((R.ROLL in kinds) == (f in (2, 4)))
    assert {c // 10 for c in forms.values()} >= {R.code(R.VALU, 4, f) // 10, R.code(R.VALU, 8, f) // 10}      # 8- and 16-byte vectors


# ------------------------------------------------------------------ b. forward, dense integers where blocks meet
@pytest.mark.parametrize("name", list(R.FWD_DENSE))
def test_forward_dense_every_form(name):
    (B, H, W, N, factors), hk, want, _ = R.FWD_DENSE[name]
    zs, add, ref, ref2 = R.fwd_dense_problem(name)
    check_forward_forms(B, H, W, N, factors, zs, [(None, False, ref), (add, True, ref2)], f"forward {name}", designed=(hk, want))


# ------------------------------------------------------------------ c. forward with statistics
@pytest.mark.parametrize("roll", [1, 0], ids=["rolling-window", "version2"])
@pytest.mark.parametrize("shape", R.FWD_STATS)
def test_forward_with_statistics(shape, roll):
    """resize_conv3x3_fwd_sum_bn: output bits, the exact mean (the sum of the outputs is an f32 value), and the variance at the
    suite's f32 tolerance against the float64 variance of the stored outputs (E[x^2] - m^2 in double: not claimed exact)."""
    B, H, W, N = shape
    zs, add, ref, _ = R.fwd_dense_problem((B, H, W, N, (2,)), -1, 1)
    out64 = ref + add
    zd, addd = [z.to(DEV, torch.bfloat16) for z in zs], add.float().to(DEV)
    with hooks(roll=roll):
        code = plan(zd, (H, W), stats=True)
        assert code == (R.code(R.ROLL, 1, 1) if roll else R.code(R.V2, 1, 1)), code
        out, mean, var = fwd_sum_bn(zd, (H, W), addd)
    R.assert_same(out, R.to_bf16_rne(out64), f"statistics variant {shape} roll={roll}: output")
    flat = out64.reshape(-1, N)
    R.assert_same(mean, flat.mean(0).float(), "mean")
    v64 = flat.var(0, unbiased=False)
    assert not var.isnan().any()
    err = (var.cpu().double() - v64).abs().max().item()
    assert err <= 1e-4 * max(v64.abs().max().item(), 1e-6), (err, v64.abs().max().item())      # test_hip_ops.close(..., torch.float32, ...)


# ------------------------------------------------------------------ d. backward gather, exhaustive basis
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("f,in_size", R.BWD_BASIS + R.BWD_BASIS_EXTRA, ids=[f"x{f}-{h}x{w}" for f, (h, w) in R.BWD_BASIS + R.BWD_BASIS_EXTRA])
def test_backward_basis_every_form(f, in_size, dtype):
    """One unit impulse per (batch, channel) over all output pixels: each of the nine maps of a channel is one row of the
    operator.  (2, 13) at x4: Wi % 4 != 0, the matrix-core block of four low-resolution pixels is partial at the end."""
    dy, ref = R.bwd_basis_problem(f, in_size)
    dyd, want = dy.to(DEV, dtype), R.expected(ref, dtype)
    forms = R.gather_forms(dtype, f)
    assert ("one-pass-mfma" in [n for n, _, _ in forms]) == (dtype == torch.bfloat16 and f in (2, 4))
    for form in forms:
        R.assert_same(gather(dyd, in_size, form), want, f"backward basis x{f} {in_size} {form[0]}")


# ------------------------------------------------------------------ e. backward gather, dense
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", R.BWD_DENSE, ids=["x".join(map(str, s)) for s in R.BWD_DENSE])
def test_backward_dense_every_form(shape, dtype):
    B, Hi, Wi, N, f = shape
    dy, ref = R.bwd_dense_problem(*shape)
    dyd, want = dy.to(DEV, dtype), R.expected(ref, dtype)
    for form in R.gather_forms(dtype, f):
        R.assert_same(gather(dyd, (Hi, Wi), form), want, f"backward dense {shape} {form[0]}")


# ------------------------------------------------------------------ f. BatchNorm-backward-fused gather
@pytest.mark.parametrize("shape", R.BN_SHAPES, ids=["x".join(map(str, s)) for s in R.BN_SHAPES])
@pytest.mark.parametrize("case,relu", [(c, r) for c in R.BN_CASES for r in ((True,) if c == "iv" else (True, False))],
                         ids=[f"{c}-{'relu' if r else 'linear'}" for c in R.BN_CASES for r in ((True,) if c == "iv" else (True, False))])
def test_bn_fused_gather(case, relu, shape):
    """ops.resize_conv3x3_bwd_gather_bn with dyadic constants (mean 0, var 1, eps 0): (i) sign flips and the ReLU mask,
    (ii) c3 = a k1, (iii) c2 = a k2 times x, (iv) thr = -1 with x = -1 exactly on the threshold (x a > thr is false there)."""
    B, Hi, Wi, N, f = shape
    p = R.bn_problem(case, shape, relu)
    bf = torch.bfloat16
    dzd, xd = p["dz"].to(DEV, bf), p["x"].to(DEV, bf)
    mean, var = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
    gamma, beta, dgs, dbs = (p[k].float().to(DEV) for k in ("gamma", "beta", "dgamma_sum", "dbeta_sum"))     # (alive across the launch)
    want = R.to_bf16_rne(p["ref"])
    assert ops.resize_conv3x3_bwd_gather_bn_ok(dzd, (Hi, Wi))
    g, coef = nans((B, Hi, Wi, 9 * N), bf), nans((4 * N,), torch.float32)
    _lib.checked().gdl_resize_conv3x3_bwd_gather_bn(dzd.data_ptr(), xd.data_ptr(), R.BF16, B, f * Hi, f * Wi, N, g.data_ptr(), Hi, Wi,
                                                    mean.data_ptr(), var.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 0.0, int(relu),
                                                    dgs.data_ptr(), dbs.data_ptr(), p["P"], coef.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    a, thr, c2, c3 = p["coefs"]
    R.assert_same(coef.view(N // 8, 4, 8).permute(1, 0, 2).reshape(4, N).cpu(), torch.stack([a, thr, c2, c3]).float(),
                  f"bn ({case}) coefficients")
    R.assert_same(g, want, f"bn ({case}) {shape} relu={relu}: fused gather")
    g2 = ops.resize_conv3x3_bwd_gather_bn(dzd, xd, (Hi, Wi), mean, var, gamma, beta, 0.0, relu, dgs, dbs, p["P"])
    R.assert_same(g2, want, f"bn ({case}) {shape} relu={relu}: ops.resize_conv3x3_bwd_gather_bn")
    R.assert_same(ops.resize_conv3x3_bwd_gather(R.to_bf16_rne(p["dy"]).to(DEV), (Hi, Wi)), want,
                  f"bn ({case}) {shape} relu={relu}: plain gather of the materialised gradient")


# ------------------------------------------------------------------ g. the plain resamplers, one node end to end
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", R.RESAMPLE, ids=["x".join(map(str, s)) for s in R.RESAMPLE])
def test_plain_resamplers(case, dtype):
    """ops.bilinear, ops.bilinear_sum and ops.bilinear_bwd at integer factors against interp_matrix on both sides."""
    hi, wi, f, Cc = case
    x, up, dout, down = R.resample_problem(*case)
    xd = x.to(DEV, dtype)
    size = (f * hi, f * wi)
    R.assert_same(ops.bilinear(xd, size, out=nans((2, *size, Cc), dtype)), R.expected(up, dtype), f"bilinear {case}")
    R.assert_same(ops.bilinear_sum([xd], size), R.expected(up, dtype), f"bilinear_sum, one source {case}")
    x2 = R.ints((2, 2 * hi, 2 * wi, Cc), 77) if f == 4 else R.ints((2, hi, wi, Cc), 77)
    both = up + R.resize_ref(x2, size[0] // x2.shape[1])
    R.assert_exact([x, x2], 1.0 / (2 * f) ** 2, [R.resize_ref(x.abs(), f) + R.resize_ref(x2.abs(), size[0] // x2.shape[1])], what="bilinear_sum")
    R.assert_same(ops.bilinear_sum([xd, x2.to(DEV, dtype)], size), R.expected(both, dtype), f"bilinear_sum, two sources {case}")
    R.assert_same(ops.bilinear_bwd(dout.to(DEV, dtype), (hi, wi), din=nans((2, hi, wi, Cc), dtype)), R.expected(down, dtype),
                  f"bilinear_bwd {case}")


def test_resized_conv_node_end_to_end():
    """conv3x3(pad 1)(bilinear x4 (x)) through the neck's low-resolution path (nn._cba_conv / nn._cba_grads: tap products as a
    1x1 GEMM, gather-sum; gathered maps, data and weight gradient as GEMMs), x, w, dy in -1..1, C = N = 64, 4 x 6 -> 16 x 24.
    The bound closes at x4 (resize_exact_ref.node_problem): forward, dx_lo and dw are bit-exact against a reference that
    rounds the gathered maps to bf16 where the kernels store them."""
    p = R.node_problem(4)
    bf = torch.bfloat16
    xd, wd, dyd = p["x"].to(DEV, bf), p["w"].float().to(DEV), p["dy"].to(DEV, bf)
    # the low-resolution path with statistics, on the rolling window: asserted, not assumed
    size = p["size"]
    assert gnn.FUSE_TAPSUM and gnn.FUSE_TAPSUM_STATS and ops.resize_conv3x3_fwd_ok((4, 6), size, 2) and ops.resize_conv3x3_fwd_bn_ok(bf, 64, None)
    hs, ws = (C.c_int * 3)(4, 1, 1), (C.c_int * 3)(6, 1, 1)
    assert _lib.load().gdl_resize_conv3x3_fwd_sum_plan(hs, ws, 1, R.BF16, 2, 64, size[0], size[1], 1) == R.code(R.ROLL, 2, 3)
    y, stats = gnn._cba_conv(xd, wd, None, 1, 4, None, None, None, 0.1)
    R.assert_same(y, R.to_bf16_rne(p["y"]), "node forward")
    assert stats is not None, "the gather-sum of the low-resolution forward emits the batch statistics"
    R.assert_same(stats[0], p["mean"].float(), "node forward: mean of the stored outputs")
    err = (stats[1].cpu().double() - p["var"]).abs().max().item()
    assert err <= 1e-4 * p["var"].max().item(), (err, p["var"].max().item())      # E[x^2] - m^2 from f32 partial sums: not claimed exact
    # the same tap products through the plain gather-sum, on the pixel-by-pixel kernel
    z = ops.conv_gemm(xd, gnn.tap_weight(wd, bf))
    with hooks(mfma=0):
        assert plan([z], size) == R.code(R.VALU, 8, 4)
        y0 = fwd_sum([z], size)
    R.assert_same(y0, R.to_bf16_rne(p["y"]), "node forward, pixel-by-pixel gather-sum")
    for form in R.gather_forms(bf, 4):
        with hooks(gather_mfma=form[1], two_pass=form[2]):
            dx, dw = gnn._cba_grads(xd, wd, dyd, 1, 4, True, True)
        R.assert_same(dx, R.to_bf16_rne(p["dx"]), f"node dx_lo ({form[0]} gather)")
        R.assert_same(dw.contiguous(), p["dw"].float(), f"node dw ({form[0]} gather)")
