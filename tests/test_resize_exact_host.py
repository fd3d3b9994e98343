"""CPU side of the exact tests of the resized-conv gather kernels: the float64 references of tests/resize_exact_ref.py against
torch's own interpolate / pad / slice and its autograd, the adjoint identity, the exactness proof (assert_exact) of EVERY case
table test_hip_resize_exact.py runs -- a case that could not be exact fails here, before anyone runs it on a GPU -- and the
forward's kernel choice (gdl_resize_conv3x3_fwd_sum_plan, a host-only query) against its mirror at every designed shape."""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import resize_exact_ref as R


def torch_fwd_sum(zs, size):
    """The definition through torch: per tap, interpolate -> zero pad -> slice."""
    H, W = size
    B, N = zs[0].shape[0], zs[0].shape[3] // 9
    out = torch.zeros(B, N, H, W, dtype=torch.float64)
    for z in zs:
        zt = z.view(B, z.shape[1], z.shape[2], 9, N).permute(0, 3, 4, 1, 2)
        for t in range(9):
            up = F.pad(F.interpolate(zt[:, t], size=(H, W), mode="bilinear", align_corners=False), (1, 1, 1, 1))
            out = out + up[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W]
    return out.permute(0, 2, 3, 1)


# (output size, factors): f in {2, 4, 8}, one to three sources, non-square maps, h = 1
GEOMETRIES = [((8, 16), (2,)), ((8, 24), (4,)), ((8, 16), (8,)), ((16, 8), (8, 4)), ((8, 24), (2, 4, 8)), ((2, 6), (2,)), ((4, 12), (4,)),
              ((24, 8), (2, 8))]


@pytest.mark.parametrize("size,factors", GEOMETRIES)
def test_interp_matrix_and_forward_reference_against_torch(size, factors):
    H, W = size
    zs = [R.ints((2, H // f, W // f, 9 * 3), 10 + f).mul(0.37) for f in factors]          # (no need for integers here)
    ref, want = R.fwd_sum_ref(zs, size), torch_fwd_sum(zs, size)
    assert (ref - want).abs().max().item() <= 1e-12
    for f in factors:
        x = torch.randn(1, 1, H // f, 1, dtype=torch.float64, generator=torch.Generator().manual_seed(f))
        up = F.interpolate(x, size=(H, 1), mode="bilinear", align_corners=False)[0, 0, :, 0]
        assert (R.interp_matrix(H // f, f) @ x[0, 0, :, 0] - up).abs().max().item() <= 1e-12


@pytest.mark.parametrize("size,factors", GEOMETRIES)
def test_gather_reference_is_the_autograd_transpose(size, factors):
    H, W = size
    for f in factors:
        z = R.ints((2, H // f, W // f, 9 * 3), 20 + f).requires_grad_(True)
        dy = R.ints((2, H, W, 3), 21 + f)
        (gz,) = torch.autograd.grad((torch_fwd_sum([z], size) * dy).sum(), z)
        g = R.bwd_gather_ref(dy, (H // f, W // f))
        # d/dz has tap block t, the kernels' layout 8 - t
        want = gz.view(2, H // f, W // f, 9, 3).flip(3).reshape(g.shape)
        assert (g - want).abs().max().item() <= 1e-12
        # <fwd(z), dy> == <z, gather(dy)>, exactly: integers times dyadic weights in float64
        zi = z.detach()
        lhs = (R.fwd_sum_ref([zi], size) * dy).sum().item()
        rhs = (zi.view(2, H // f, W // f, 9, 3).flip(3).reshape(g.shape) * g).sum().item()
        assert lhs == rhs
        rows = R.bwd_rows_ref(dy, H // f)
        assert rows.shape == (3, 2, H // f, W, 3)


def test_bn_formula_is_the_batchnorm_relu_backward():
    """bn_dy_ref with the constants of bn_coefs against autograd of relu(batch_norm(x)) where the batch statistics are the
    ones the constants assume (mean 0, var 1 -- enforced by construction of x)."""
    g = torch.Generator().manual_seed(3)
    P, N = 64, 4
    x = torch.randn(P, N, dtype=torch.float64, generator=g)
    x = (x - x.mean(0)) / x.var(0, unbiased=False).sqrt()
    dz = torch.randn(P, N, dtype=torch.float64, generator=g)
    gamma, beta = torch.tensor([1.0, 2.0, -1.0, 0.5], dtype=torch.float64), torch.tensor([0.0, 0.3, -0.2, 1.0], dtype=torch.float64)
    for relu in (True, False):
        xr = x.clone().requires_grad_(True)
        y = F.batch_norm(xr, None, None, gamma, beta, True, 0.1, 1e-30)
        y = F.relu(y) if relu else y
        (want,) = torch.autograd.grad(y, xr, dz)
        dzm = torch.where((x * gamma + beta > 0) | (not relu), dz, torch.zeros_like(dz))
        k1, k2 = dzm.mean(0), (dzm * x).mean(0)
        got = R.bn_dy_ref(dz, x, *R.bn_coefs(gamma, beta, relu, k1, k2))
        assert (got - want).abs().max().item() <= 1e-12


def test_assert_exact_rejects_what_is_not_exact():
    q = 1.0 / 64
    ok = R.ints((4, 4), 1)
    R.assert_exact([ok], q, [ok.abs()], stored=[ok * 0.5])
    with pytest.raises(AssertionError, match="integers"):
        R.assert_exact([ok * 0.5], q, [ok.abs()])
    with pytest.raises(AssertionError, match="2\\^24"):
        R.assert_exact([ok], q, [ok.abs() * 2.0 ** 18 + 1])
    with pytest.raises(AssertionError, match="stores in bf16"):
        R.assert_exact([ok], q, [ok.abs()], stored=[ok + 1.0 / 512])
    with pytest.raises(AssertionError, match="bf16 values"):
        R.assert_exact([ok * 257], q, [ok.abs()])
    with pytest.raises(AssertionError):
        R.to_bf16_rne(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
    assert R.to_bf16_rne(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)).tolist() == [1.0, 1.015625]   # ties to even


# ------------------------------------------------------------------ every GPU case table is exact
@pytest.mark.parametrize("f", list(R.FWD_BASIS))
def test_forward_basis_cases_are_exact(f):
    z, ref = R.fwd_basis_problem(f)
    h, w = R.FWD_BASIS[f]
    assert z.shape[0] * R.BASIS_N >= h * w * 9 and z.sum().item() == h * w * 9
    # the reference IS the operator, column by column
    uy, ux = R.interp_matrix(h, f), R.interp_matrix(w, f)
    for i in (0, h * w * 9 // 2, h * w * 9 - 1):
        pix, tap = divmod(i, 9)
        col = torch.outer(R.shifted(uy, tap // 3 - 1)[:, pix // w], R.shifted(ux, tap % 3 - 1)[:, pix % w])
        assert torch.equal(ref[i // R.BASIS_N, :, :, i % R.BASIS_N], col)


@pytest.mark.parametrize("name", [n for n in R.FWD_DENSE if n != "roll-second-column"])
def test_forward_dense_cases_are_exact(name):
    zs, add, ref, ref2 = R.fwd_dense_problem(name)
    assert ref.shape == ref2.shape and (ref2 >= 0).all()
    R.to_bf16_rne(ref), R.to_bf16_rne(ref2)


def test_forward_dense_largest_case_is_exact():
    """(65, 32, 40, 256, x4): the one large reference, about a second of einsums."""
    zs, add, ref, ref2 = R.fwd_dense_problem("roll-second-column")
    R.to_bf16_rne(ref), R.to_bf16_rne(ref2)


@pytest.mark.parametrize("shape", R.FWD_STATS)
def test_forward_statistics_cases_are_exact(shape):
    B, H, W, N = shape
    zs, add, ref, _ = R.fwd_dense_problem((B, H, W, N, (2,)), -1, 1)
    out = ref + add
    assert R.is_bf16(out), "every output is a bf16 value: the statistics of the f32 sums and of the stored outputs coincide"
    q = 1.0 / 16
    assert out.abs().sum((0, 1, 2)).max().item() / q < R.EXACT                    # the sum of the outputs: exact in f32
    assert (out * out).sum((0, 1, 2)).max().item() / (q * q) < 2.0 ** 53


@pytest.mark.parametrize("f,in_size", R.BWD_BASIS + R.BWD_BASIS_EXTRA)
def test_backward_basis_cases_are_exact(f, in_size):
    dy, ref = R.bwd_basis_problem(f, in_size)
    assert dy.sum().item() == f * f * in_size[0] * in_size[1]
    if (f, in_size) in R.BWD_BASIS:
        assert tuple(dy.shape) == (2, 8, 16, 64)
    # every map sums the weights of its tap: a dropped or doubled border contribution changes the total
    assert ref.sum().item() > 0


@pytest.mark.parametrize("shape", R.BWD_DENSE)
def test_backward_dense_cases_are_exact(shape):
    dy, ref = R.bwd_dense_problem(*shape)
    R.to_bf16_rne(ref)


@pytest.mark.parametrize("shape", R.BN_SHAPES)
@pytest.mark.parametrize("case", R.BN_CASES)
def test_bn_fused_cases_are_exact(case, shape):
    for relu in ((True,) if case == "iv" else (True, False)):
        p = R.bn_problem(case, shape, relu)
        R.to_bf16_rne(p["ref"])
        a, thr, c2, c3 = p["coefs"]
        for c in (a, c2, c3):
            assert torch.equal(c.float().double(), c)
        if case == "iv":
            masked = (p["x"] == -1) & (p["dz"] != 0)
            assert masked.any() and torch.equal(p["dy"][masked], torch.zeros(int(masked.sum()), dtype=torch.float64))
        if relu and case != "iv":
            assert (p["dy"] == 0).any() and (p["dy"] != 0).any()


@pytest.mark.parametrize("case", R.RESAMPLE)
def test_resampler_cases_are_exact(case):
    x, up, dout, down = R.resample_problem(*case)
    f = case[2]
    want = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=f, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert (up - want).abs().max().item() <= 1e-12
    assert (up * dout).sum().item() == (x * down).sum().item()
    for t in (up, down):
        R.to_bf16_rne(t)


def test_node_case_is_exact_at_factor_4():
    p = R.node_problem(4)
    x, w, dy = p["x"], p["w"], p["dy"]
    xr, wr = x.permute(0, 3, 1, 2).clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(F.interpolate(xr, size=p["size"], mode="bilinear", align_corners=False), wr, padding=1)
    assert torch.equal(y.permute(0, 2, 3, 1), p["y"])                  # integers times dyadic weights: float64 is exact
    # the gradients with G unrounded are autograd's; the reference rounds G to bf16, which moves them by a little
    y.backward(dy.permute(0, 3, 1, 2))
    assert (p["dx"] - xr.grad.permute(0, 2, 3, 1)).abs().max().item() <= 2.0 ** -8 * 9 * 64 * 32
    assert (p["dw"] - wr.grad).abs().max().item() <= 2.0 ** -8 * 48 * 32
    for t in (p["y"], p["dx"]):
        R.to_bf16_rne(t)
    assert torch.equal(p["dw"].float().double(), p["dw"])


# ------------------------------------------------------------------ the planner
@pytest.fixture(scope="module")
def lib():
    from gdlhip import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def query(lib, B, H, W, N, factors, dtype, stats=False, mfma=1, vec=0, roll=1, persist=1):
    n = len(factors)
    hs = (C.c_int * 3)(*([H // f for f in factors] + [1] * (3 - n)))
    ws = (C.c_int * 3)(*([W // f for f in factors] + [1] * (3 - n)))
    lib.gdl_debug_set_tapsum_mfma(mfma), lib.gdl_debug_set_tapsum_vec(vec), lib.gdl_debug_set_tapsum_roll(roll)
    lib.gdl_debug_set_tapsum_persist(persist)
    try:
        return lib.gdl_resize_conv3x3_fwd_sum_plan(hs, ws, n, dtype, B, N, H, W, int(stats))
    finally:
        lib.gdl_debug_set_tapsum_mfma(1), lib.gdl_debug_set_tapsum_vec(0), lib.gdl_debug_set_tapsum_roll(1)
        lib.gdl_debug_set_tapsum_persist(1)


def test_plan_query_equals_its_mirror_at_every_designed_shape(lib):
    """No GPU: the query is host arithmetic and counts on 256 CUs until a launch has seen the device."""
    shapes = [(s, hooks, want) for s, hooks, want, _ in R.FWD_DENSE.values()]
    shapes += [((-(-h * w * 9 // 64), *R.BASIS_OUT, R.BASIS_N, (f,)), {}, None) for f, (h, w) in R.FWD_BASIS.items()]
    for (B, H, W, N, factors), hooks, want in shapes:
        if want is not None:
            assert query(lib, B, H, W, N, factors, R.BF16, **hooks) == want == R.plan_mirror(factors, R.BF16, B, N, H, W, **hooks), (B, H, W, N, factors)
        forms = R.forms_of(B, H, W, N, factors)
        assert "production" in forms and "valu-f32" in forms
        for name, c in forms.items():
            dtype, h = R.FORMS[name]
            assert query(lib, B, H, W, N, factors, R.BF16 if dtype == torch.bfloat16 else R.F32, **h) == c, (name, B, H, W, N, factors)
    for B, H, W, N in R.FWD_STATS:
        for roll in (1, 0):
            got = query(lib, B, H, W, N, (2,), R.BF16, stats=True, roll=roll)
            assert got == R.plan_mirror((2,), R.BF16, B, N, H, W, stats=True, roll=roll) == (R.code(R.ROLL, 1, 1) if roll else R.code(R.V2, 1, 1))


def test_plan_query_literal_codes_and_refusals(lib):
    q = lambda *a, **k: query(lib, *a, **k)      # noqa: E731
    assert q(2, 8, 16, 64, (2,), R.F32) == 420 and q(2, 8, 16, 64, (8,), R.F32) == 480                    # VALU f32: vec 4, run
    assert q(2, 8, 16, 64, (8,), R.BF16, mfma=0) == 480 and q(2, 8, 16, 64, (8,), R.BF16, mfma=0, vec=8) == 880
    assert q(2, 8, 16, 64, (4,), R.BF16, mfma=0) == 840 and q(2, 8, 16, 64, (4,), R.BF16, mfma=0, vec=4) == 440
    assert q(2, 8, 16, 64, (4,), R.BF16) == 3230 and q(2, 8, 16, 64, (4,), R.BF16, roll=2) == 3210 and q(2, 8, 16, 64, (2,), R.BF16) == 3110
    assert q(2, 8, 16, 64, (4,), R.BF16, roll=0) == 2120 and q(2, 8, 16, 64, (2,), R.BF16, roll=0) == 1100
    assert q(2, 8, 16, 64, (4,), R.BF16, mfma=2) == 1200 and q(2, 8, 16, 64, (4,), R.BF16, mfma=4) == 1100
    assert q(2, 8, 16, 64, (8, 4), R.BF16, mfma=5) == 2200 and q(2, 8, 16, 64, (2, 4, 8), R.BF16, mfma=5) == 2300
    assert q(2, 8, 16, 64, (2, 4, 8), R.BF16) == 4320 and q(2, 8, 16, 64, (4, 2, 8), R.BF16) == 1100       # roll3 wants 2, 4, 8 in order
    assert q(2, 8, 16, 64, (2, 4, 8), R.BF16, stats=True) == 2300
    # persistent grid: 3 * 256 workgroups stay resident for one source, 256 for several
    assert q(4, 64, 192, 64, (4,), R.BF16, roll=0) == 2120 and q(4, 64, 208, 64, (4,), R.BF16, roll=0) == 2121
    assert q(4, 64, 208, 64, (4,), R.BF16, roll=0, persist=0) == 2120
    # refused: a factor of 3, unequal factors, Wo no multiple of the largest factor, statistics without the matrix cores
    assert q(1, 9, 9, 64, (3,), R.BF16) == -1 and q(1, 8, 12, 64, (8,), R.BF16) == -1
    assert q(1, 8, 16, 72, (2,), R.BF16, stats=True) == -1 and q(1, 8, 16, 64, (2,), R.F32, stats=True) == -1
    assert b"statistics" in lib.gdl_last_error() or b"fwd_sum_bn" in lib.gdl_last_error()
    hs = (C.c_int * 3)(4, 1, 1)
    assert lib.gdl_resize_conv3x3_fwd_sum_plan(hs, hs, 0, R.BF16, 1, 64, 8, 8, 0) == -1
    assert lib.gdl_resize_conv3x3_fwd_sum_plan(None, hs, 1, R.BF16, 1, 64, 8, 8, 0) == -1
