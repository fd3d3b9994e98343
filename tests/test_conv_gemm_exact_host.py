"""The references, bound helpers, tile-order mirror and shape tables of tests/test_hip_conv_gemm_exact.py, tested where there is
no GPU: the integer forward and data-gradient references against naive loops on a 2 x 3 x 3 example, the epilogue reference
against a scalar loop, the 2^24 and 2^8 bounds, the conv_n_group mirror against hand-worked values, and every case of every
table -- its tile counts, K-step counts and tails are what its comment says, its operands satisfy the 2^24 bound, its bf16
reference stays within 2^8 -- computed from the same seeded operands the GPU tests use."""

import pytest
import torch

import test_hip_conv_gemm_exact as ex

BF16, F32 = ex.BF16, ex.F32


# ------------------------------------------------------------------ references against naive loops
def naive_conv(x, w4, stride, pad):
    B, H, W, Cc = x.shape
    N, _, R, S = w4.shape
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    y = torch.zeros(B, Ho, Wo, N, dtype=torch.int64)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for r in range(R):
                    for s in range(S):
                        iy, ix = oy * stride + r - pad, ox * stride + s - pad
                        if 0 <= iy < H and 0 <= ix < W:
                            for n in range(N):
                                for c in range(Cc):
                                    y[b, oy, ox, n] += int(x[b, iy, ix, c]) * int(w4[n, c, r, s])
    return y.double()


def naive_dgrad(dy, w4, stride, pad, hw):
    B, Ho, Wo, N = dy.shape
    _, Cc, R, S = w4.shape
    dx = torch.zeros(B, *hw, Cc, dtype=torch.int64)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for r in range(R):
                    for s in range(S):
                        iy, ix = oy * stride + r - pad, ox * stride + s - pad
                        if 0 <= iy < hw[0] and 0 <= ix < hw[1]:
                            for n in range(N):
                                for c in range(Cc):
                                    dx[b, iy, ix, c] += int(dy[b, oy, ox, n]) * int(w4[n, c, r, s])
    return dx.double()


@pytest.mark.parametrize("R,S,stride,pad", [(1, 1, 1, 0), (3, 3, 1, 1), (3, 3, 2, 1), (2, 2, 2, 0), (3, 1, 1, 1)])
def test_integer_references_match_naive_loops(R, S, stride, pad):
    B, H, W, Cc, N = 2, 3, 3, 3, 2
    x, w4 = ex.ints((B, H, W, Cc), 1), ex.ints((N, Cc, R, S), 2)
    y = naive_conv(x, w4, stride, pad)
    assert y.abs().max() > 0
    assert torch.equal(ex.ref_conv(x, w4, stride, pad), y)
    dy = ex.ints(tuple(y.shape), 3)
    dx = naive_dgrad(dy, w4, stride, pad, (H, W))
    assert dx.abs().max() > 0
    assert torch.equal(ex.ref_dgrad(dy, w4, stride, pad, (H, W)), dx)
    # the kernels' weight layout [N, (r, s, c)]
    wm = ex.gemm_weights(w4)
    assert wm.shape == (N, R * S * Cc) and all(wm[1, (r * S + s) * Cc + c] == w4[1, c, r, s]
                                               for r in range(R) for s in range(S) for c in range(Cc))


def test_big_problem_matches_the_float64_reference():
    g = ex.geo(2, 1, 37, 64, 24)
    x, w, acc = ex.big_problem(g, 4)
    want = ex.ref_conv(x.double().view(2, 1, 37, 64), w.double().view(24, 64, 1, 1), 1, 0)
    assert torch.equal(acc.double().view(2, 1, 37, 24), want) and acc.abs().max() > 0
    assert set(x.unique().tolist()) == {-1.0, 0.0, 1.0} and 0.15 < (x != 0).float().mean().item() < 0.35


# ------------------------------------------------------------------ the epilogue reference against a scalar loop
@pytest.mark.parametrize("name", list(ex.EPIS))
def test_epilogue_reference_matches_a_scalar_loop(name):
    B, Ho, Wo, N = 3, 2, 2, 5
    acc = ex.ints((B, Ho, Wo, N), 11, -20, 20)
    e = ex.make_epi(name, B, Ho, Wo, N)
    got = ex.ref_epilogue(acc, e)
    sc, sh, act, bs, rs = ex.EPIS[name]
    assert (e["scale"] is not None, e["shift"] is not None, e["batch_scale"] is not None, e["resid"] is not None) == \
        (bool(sc), bool(sh), bool(bs), bool(rs))
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for n in range(N):
                    v = acc[b, oy, ox, n].item() + e["bias"][n].item()
                    if sc:
                        v = v * e["scale"][n].item() + (e["shift"][n].item() if sh else 0.0)
                    if act == "relu":                       # before the DropPath scale and the residual
                        v = max(v, 0.0)
                    if bs:
                        v *= e["batch_scale"][b].item()
                    if rs:
                        v += e["resid"][b, oy, ox, n].item()
                    if act == "resid_relu":                 # after the residual
                        v = max(v, 0.0)
                    assert got[b, oy, ox, n].item() == v, (name, b, oy, ox, n)
    # the ReLU position matters on these operands: moving it changes the result
    if act == "relu" and rs:
        moved = dict(e, act="resid_relu")
        assert not torch.equal(ex.ref_epilogue(acc, moved), got)


def test_channel_constants_differ_from_their_neighbours():
    N = 512
    for vec in (ex.chan_bias(N), ex.chan_scale(N), ex.chan_shift(N)):
        for d in (1, 4, 16, 64):
            assert (vec[d:] != vec[:-d]).all(), d
    assert ex.chan_bias(N).abs().max() == 9 and set(ex.chan_scale(N).tolist()) == set(ex.SCALES)
    assert ex.batch_scales(3).tolist() == [2.0, 0.0, 1.0]


# ------------------------------------------------------------------ the bounds
def test_exact_bound_raises_at_the_bound_and_on_non_integers():
    x, w = torch.full((4,), 2.0, dtype=torch.float64), torch.full((4,), -2.0, dtype=torch.float64)
    assert ex.assert_exact_bound(x, w, 1000) == 4000
    assert ex.assert_exact_bound(x, w, (1 << 22) - 1) == (1 << 24) - 4
    with pytest.raises(AssertionError):
        ex.assert_exact_bound(x, w, 1 << 22)                           # 4 K = 2^24: the largest partial sum may round
    with pytest.raises(AssertionError):
        ex.assert_exact_bound(x * 0.75, w, 10)                         # not integers
    one = torch.ones(1, dtype=torch.float64)
    e = dict(bias=9 * one, scale=4 * one, shift=8 * one, batch_scale=2 * one, resid=9 * one)
    assert ex.assert_exact_bound(x, w, 100, e) == ((400 + 9) * 4 + 8) * 2 + 9
    # every epilogue term counts: K chosen so that the accumulator alone passes and one more term reaches 2^24
    K = (1 << 22) - 1                                                  # 4 K = 2^24 - 4
    assert ex.assert_exact_bound(x, w, K, dict(bias=3 * one)) == (1 << 24) - 1
    for bad in (dict(bias=4 * one), dict(scale=2 * one), dict(bias=0 * one, scale=one, shift=4 * one),
                dict(batch_scale=2 * one), dict(resid=4 * one), dict(bias=0.5 * one)):
        with pytest.raises(AssertionError):
            ex.assert_exact_bound(x, w, K, bad)


def test_bf16_bound_raises_past_256_and_on_non_integers():
    assert ex.assert_bf16_exact(torch.tensor([-256.0, 3.0, 256.0])) == 256
    with pytest.raises(AssertionError):
        ex.assert_bf16_exact(torch.tensor([257.0]))                    # 257 is not a bf16 value
    with pytest.raises(AssertionError):
        ex.assert_bf16_exact(torch.tensor([0.5]))
    assert torch.equal(torch.arange(-256, 257).float().bfloat16().float(), torch.arange(-256, 257).float())
    assert torch.tensor([257.0]).bfloat16().float().item() != 257.0


# ------------------------------------------------------------------ the conv_n_group mirror
def test_conv_n_group_mirror_hand_worked():
    # bf16 C = 64: 128 bytes of K per row; a 256-row panel is 32 KiB.  N = 2048: 8 N tiles of 256.
    # 96 KiB: 3 panels fit.  cost(3) = (32 // 3) * 32 KiB + 0 = 320 KiB  <  cost(8) = (32 // 8) * 32 KiB + 8 * 32 KiB = 384 KiB:
    # ceil(8 / 3) = 3 groups of ceil(8 / 3) = 3 -> widths 3, 3, 2.
    assert ex.conv_n_group(1, 1, 64, 2, 2048, 256, 256, 32, 96) == 3
    # the dual tile: 128-row weight panels of 16 KiB, 16 N tiles, 64 resident tiles per XCD.  6 fit.  cost(6) = (64 // 6) * 32 KiB
    # = 320 KiB  <  cost(16) = 4 * 32 KiB + 16 * 16 KiB = 384 KiB: 3 groups of ceil(16 / 3) = 6 -> widths 6, 6, 4.
    assert ex.conv_n_group(1, 1, 64, 2, 2048, 256, 128, 64, 96) == 6
    # 128 KiB: 4 fit, cost(4) = 8 * 32 KiB = 256 KiB < 384 KiB: two groups of four (not ragged)
    assert ex.conv_n_group(1, 1, 64, 2, 2048, 256, 256, 32, 128) == 4
    # the default budget holds all eight panels, 16 KiB holds none, 0 switches grouping off: no grouping
    assert ex.conv_n_group(1, 1, 64, 2, 2048, 256, 256, 32, 2560) == 0
    assert ex.conv_n_group(1, 1, 64, 2, 2048, 256, 256, 32, 16) == 0
    assert ex.conv_n_group(1, 1, 64, 2, 2048, 256, 256, 32, 0) == 0
    # 32 KiB: one panel fits, cost(1) = 32 * 32 KiB = 1 MiB >= 384 KiB: grouping would cost more than it saves
    assert ex.conv_n_group(1, 1, 64, 2, 2048, 256, 256, 32, 32) == 0
    # what the GPU test relies on
    for variant, width in ((3, 3), (8, 3), (9, 3), (6, 6)):
        bm, bn = ex.TILE[variant]
        g = ex.G_NGROUP
        assert ex.conv_n_group(1, 1, g.C, 2, g.N, bm, bn, ex.NGROUP_CONC[variant], ex.NGROUP_KB) == width
        assert ex.facts(g, BF16, variant)["tiles_n"] % width != 0 and ex.facts(g, BF16, variant)["m_tail"] == 37


# ------------------------------------------------------------------ the shape tables
def check_case(g, dtype, wide, e, out_dtype):
    """What ex.run asserts on the reference side of a case."""
    x, w4, acc = ex.problem(g, wide)
    ex.assert_exact_bound(x, w4, g.R * g.S * g.C, e)
    if out_dtype == BF16:
        ex.assert_bf16_exact(ex.ref_epilogue(acc, e))


def test_tables_of_the_256_tiles():
    for row in ex.T256:
        for dtype in (BF16, F32):
            g = ex.t256_geo(row, dtype)
            f = ex.facts(g, dtype, 3)
            assert {k: f[k] for k in row[-1]} == row[-1], row[0]
            assert g.C % ex.BKE[dtype] == 0 and g.N % 256 == 0 and f["m_tail"] != 0
            check_case(g, dtype, True, dict(bias=ex.chan_bias(g.N)), F32)
    assert sorted(r[-1]["ksteps"] for r in ex.T256 if r[6] == 1) == [1, 2, 3, 5]        # 1, 2, 3 and an odd count above 4
    assert {r[5] for r in ex.T256} == {256, 512}
    # a tile spans a sample boundary in the 1x1 and the 3x3 cases
    for row in ex.T256[:5]:
        g = ex.t256_geo(row, BF16)
        Ho, Wo = ex.out_hw(g)
        assert g.B > 1 and Ho * Wo % 256 != 0 and Ho * Wo < 256


def test_table_of_the_shared_staging_tile():
    assert {r[3] for r in ex.TSF} == {5, 16, 23} and {r[2] for r in ex.TSF} >= {1, 2} and {r[4] for r in ex.TSF} == {64, 192}
    assert 288 % 16 == 0 and 288 % 23 != 0 and 5 < 288      # the kernel stages 288 pixels: W = 16 divides them, 23 does not
    for _, B, H, W, Cc, want, ksteps in ex.TSF:
        assert B == 3
        for dtype in (BF16, F32):
            g = ex.geo(B, H, W, Cc, 256, 3, pad=1)
            f = ex.facts(g, dtype, 4)
            assert {k: f[k] for k in want} == want and f["ksteps"] == ksteps[dtype == F32]
            assert g.C % ex.BKE[dtype] == 0
            check_case(g, dtype, True, dict(bias=ex.chan_bias(256)), F32)


def test_table_of_the_narrow_output_tile():
    modes = {}
    for row in ex.T5:
        _, dtype, Cc, filt, mode, kt_packed, kt_plain = row
        modes.setdefault((ex.DT_ID[dtype], mode), set()).add(Cc)
        for N in ex.T5_N:
            g = ex.t5_geo(row, N)
            assert ex.t5_mode(g, dtype, 1) == mode and ex.t5_mode(g, dtype, 0) == ("plain" if mode == "plain" else "ctail")
            assert ex.facts(g, dtype, 5, tap_packed=mode == "tap")["ksteps"] == kt_packed
            f = ex.facts(g, dtype, 5)
            assert (f["M"], f["tiles_m"], f["m_tail"], f["tiles_n"], f["ksteps"]) == (286, 2, 30, 1, kt_plain)
            check_case(g, dtype, True, dict(bias=ex.chan_bias(N)), F32)
    assert modes == {("bf16", "plain"): {64}, ("f32", "plain"): {32}, ("bf16", "ctail"): {72, 40}, ("f32", "ctail"): {36},
                     ("bf16", "tap"): {8, 16, 32}, ("f32", "tap"): {4, 8, 16}}
    assert sum(1 for r, p in ex.T5_RUNS if not p) == 12


def test_tables_of_the_dual_narrow_and_four_stage_tiles():
    for _, g, want in ex.T6:
        assert ex.facts(g, BF16, 6) == want and g.N == 200
        check_case(g, BF16, True, dict(bias=ex.chan_bias(g.N)), F32)
    for H, W in ex.T7_HW.values():
        assert H % 4 == 0 and W % 64 == 0
        for Cc in (8, 16, 32):
            for N in ex.T7_N:
                check_case(ex.geo(2, H, W, Cc, N, 3, pad=1), BF16, True, dict(bias=ex.chan_bias(N)), F32)
    assert [H // 4 * (W // 64) for H, W in ex.T7_HW.values()] == [1, 4]
    for _, g, ksteps in ex.T12:
        assert ex.facts(g, BF16, 12) == dict(M=165, tiles_m=3, m_tail=37, tiles_n=2, n_tail=8, ksteps=ksteps)
        check_case(g, BF16, True, dict(bias=ex.chan_bias(g.N)), F32)
    assert {1, 3, 4, 5} <= {r[2] for r in ex.T12} and max(r[2] for r in ex.T12) >= 27     # 1, stages - 1, stages, stages + 1, long


@pytest.mark.parametrize("variant,g,want", ex.PERSISTENT, ids=["v9", "v10-kt12", "v10-kt16"])
def test_table_of_the_persistent_tiles(variant, g, want):
    """(the accumulator as an f32 matmul on the CPU: exact under the bound)"""
    assert ex.facts(g, BF16, variant) == want
    tiles = want["tiles_m"] * want["tiles_n"]
    assert tiles > 2 * ex.MI355X_CUS and want["m_tail"] != 0
    assert tiles - 2 * ex.MI355X_CUS >= 64, "at least 64 workgroups take a third tile"
    if variant == 10:
        assert g.C % 256 == 0 and g.C >= 768 and g.N % 256 == 0
    x, w, acc = ex.big_problem(g, ex.BIG_KEEP[variant])
    acc = acc.double().view(g.B, g.H, g.W, g.N)
    N = g.N
    affine = dict(bias=ex.chan_bias(N), scale=ex.chan_scale(N), shift=ex.chan_shift(N), act="relu")
    for e in (dict(bias=ex.chan_bias(N)), affine, dict(affine, shift=None)):
        ex.assert_exact_bound(x, w, g.C, e)
        ex.assert_bf16_exact(ex.ref_epilogue(acc, e))


def test_tables_of_the_epilogue_and_k_order_cases():
    for variant, dtype in ex.EPI_TILES:
        g = ex.epi_geo(variant, dtype)
        Ho, Wo = ex.out_hw(g)
        f = ex.facts(g, dtype, variant)
        assert g.C % (16 if variant == 7 else ex.BKE[dtype]) == 0 and (variant == 7 or f["ksteps"] == g.R * g.S)
        assert g.N % ex.TILE[variant][1] == 0 and g.B == 3
        if variant == 7:
            assert Ho * Wo == 256
        else:       # a DropPath scale passes the coalesced epilogue, sample boundaries fall inside 32-row passes, M has a tail
            assert Ho * Wo == 273 and f["M"] == 819 and f["m_tail"] == 819 % ex.TILE[variant][0] != 0 and 273 % 32 != 0
        for name in ex.EPIS:
            e = ex.make_epi(name, g.B, Ho, Wo, g.N)
            for out_dtype in (F32, BF16):
                check_case(g, dtype, out_dtype == F32, e, out_dtype)
    assert {v for v, _ in ex.EPI_TILES} == set(ex.ALL_VARIANTS) - {10}
    for variant, dtype in ex.KORDER_TILES:
        g = ex.geo(2, 9, 17, 2 * ex.BKE[dtype], 64 if variant == 5 else 256, 3, pad=1)
        assert ex.facts(g, dtype, variant)["ksteps"] == 18
        check_case(g, dtype, True, dict(bias=ex.chan_bias(g.N)), F32)
    g = ex.geo(3, 13, 21, 64, 128)                                                      # aux_out
    e = dict(bias=ex.chan_bias(g.N), scale=ex.chan_scale(g.N), shift=ex.chan_shift(g.N), act="relu")
    check_case(g, BF16, False, e, BF16)
    check_case(g, BF16, False, dict(bias=e["bias"]), BF16)


@pytest.mark.parametrize("name,g,hooks,variant,pixels", ex.STATS, ids=[r[0] for r in ex.STATS])
def test_table_of_the_statistics_cases(name, g, hooks, variant, pixels):
    M = g.B * g.H * g.W
    bm, bn = ex.TILE[variant]
    assert M % bm == 0 and g.N % bn == 0 and pixels == bm // 2                           # a partial row per 32 * TM pixels
    assert (M // bm) * (g.N // bn) == (224 if variant == 1 else 480)
    x, w4, bias, y = ex.stats_problem(g)                                                # asserts both bounds
    assert y.abs().max().item() <= 256 and pixels * 256 ** 2 < ex.EXACT
