"""The tables, references and launcher mirrors of tests/test_hip_rowcol_exact.py, tested where there is no GPU: every table's
largest partial sum stays below 2^24 (bf16 operands and outputs within 2^8) on the very operands the GPU tests use, every
reference helper agrees with a naive loop, and every table row reaches the structure it is there for -- lane map, empty trailing
blocks, a batch boundary inside a block, segment tails of 1, 2 and 0 mod 3, forward block counts 1 / 7 / 8 / 9 / 17, the nblk
clamp on and off -- according to plain-Python mirrors of row_blocks, col_map, the depthwise kernels' maps, seg_len / seg_of and
the launch arithmetic.  A launcher change that moves a shape fails here instead of silently testing something else."""

import pytest
import torch
import torch.nn.functional as F

import test_hip_rowcol_exact as ex

EXACT, BF16_EXACT = ex.EXACT, 1 << 8


# ------------------------------------------------------------------ mirrors against hand-worked values
def test_row_blocks_and_partition_by_hand():
    assert [ex.row_blocks(r) for r in (1, 15, 16, 31, 32, 47, 300, 8191, 8192, 8200, 10 ** 6)] == \
        [1, 1, 1, 1, 2, 2, 18, 511, 512, 512, 512]
    assert ex.partition(300, 18) == (17, 18)          # block 17 owns rows 289..299
    assert ex.partition(289, 18) == (17, 17)          # block 17 owns nothing: the smallest row count with an empty block
    assert all(ex.partition(r, ex.row_blocks(r))[1] == ex.row_blocks(r) for r in range(1, 289))
    assert ex.partition(8192, 512) == (16, 512)
    assert ex.partition(8200, 512) == (17, 483) and ex.partition(8191, 511) == (17, 482)
    assert ex.partition(8193, 512) == (17, 482)


def test_lane_maps_by_hand():
    assert [ex.col_lanes(c) for c in (4, 16, 20, 32, 36, 64, 68, 128, 132, 768)] == [4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    assert [ex.dw_lanes(c) for c in (4, 64, 68, 128, 132, 320)] == [16, 16, 32, 32, 64, 64]
    assert [ex.ln_lanes(d) for d in (4, 64, 68, 128, 132, 256, 260, 512, 516, 1024)] == \
        [(16, 1), (16, 1), (32, 1), (32, 1), (64, 1), (64, 1), (64, 2), (64, 2), (64, 4), (64, 4)]
    for lanes in (ex.col_lanes, ex.dw_lanes):        # the lanes of a row hold all its channels of one 256-channel block
        assert all(4 * lanes(c) >= min(c, 256) for c in range(4, 1028, 4))


def test_segments_and_block_counts_by_hand():
    assert ex.segments(1) == [(0, 1)] and ex.segments(32) == [(0, 32)] and ex.segments(33) == [(0, 32), (32, 33)]
    assert ex.segments(70) == [(0, 32), (32, 64), (64, 70)]
    assert ex.dw_fwd_blocks(1, 1, 1, 4) == (1, 8) and ex.dw_fwd_blocks(2, 5, 70, 256) == (8, 8)
    assert ex.dw_fwd_blocks(2, 5, 70, 288) == (9, 16)
    assert ex.dw_bwd_blocks(2, 5, 64, 256) == (5, 40, 20)          # clamp active: 20 items / 4 waves < 640 rows / 16
    assert ex.dw_bwd_blocks(2, 5, 1, 260) == (1, 1, 10)            # 10 pixels: one block either way


# ------------------------------------------------------------------ 1. column sums
def test_colsum_tables():
    assert set(ex.COLSUM_C) == {4, 16, 20, 32, 64, 96, 128, 132, 160, 256, 260, 320, 768}
    assert {1, 3, 6, 15, 16, 17, 33, 47, 300} <= set(ex.COLSUM_ROWS)
    assert {ex.col_lanes(c) for c in ex.COLSUM_C} == {4, 8, 16, 32, 64} == {ex.col_lanes(c) for c in ex.COLSUM_LAYOUT_C}
    assert max(ex.COLSUM_C) > 512 and 260 in ex.COLSUM_C           # three and two channel blocks, the second one ragged
    # rows below one lane group of rows (4 waves x nsub), ragged last blocks, empty trailing blocks
    empties = {r: ex.row_blocks(r) - ex.partition(r, ex.row_blocks(r))[1] for r in ex.COLSUM_ROWS}
    assert empties[289] == 1 and all(v == 0 for r, v in empties.items() if r != 289), "trailing blocks empty: 289 only"
    big = {r: ex.row_blocks(r) - ex.partition(r, ex.row_blocks(r))[1] for r, _ in ex.COLSUM_BIG}
    assert big == {8191: 29, 8192: 0, 8200: 29}, "trailing blocks empty at 8191 and 8200 rows"
    assert {(8200, 32), (8200, 260)} <= set(ex.COLSUM_BIG) and all(c in (32, 260) for r, c in ex.COLSUM_BIG if r == 8200)
    for Cc in ex.COLSUM_C:                                         # the bound, on the operands themselves
        x, cum = ex.colsum_operand(Cc)
        assert x.abs().max() <= 2 and torch.equal(x, x.round()) and torch.equal(cum[-1], x.sum(0))
    assert 2 * 8200 + 100 < EXACT                                  # |v| <= 2 over at most 8200 rows on a preset of at most 100


# ------------------------------------------------------------------ 2. LayerScale backward
def test_layerscale_tables():
    assert {ex.col_lanes(c) for c in ex.LS_C} == {4, 8, 16, 32, 64} and max(ex.LS_C) > 512
    assert (3, 11) in ex.LS_BN
    per, _ = ex.partition(33, ex.row_blocks(33))
    assert ex.row_blocks(33) == 2 and per == 17 and 0 < 11 < per, "rows span a batch boundary: block 0 holds rows 0..16, batches 0 and 1"
    assert per % 11 != 0 and 33 % per != 0
    B, N, Cc = ex.LS_BIG
    assert ex.row_blocks(B * N) - ex.partition(B * N, 512)[1] == 30, "trailing blocks empty"
    seen = set()
    for form in ex.LS_FORMS:
        for Cc in ex.LS_C:
            for B, N in ex.LS_BN + [ex.LS_BIG[:2]]:
                g, z, gamma, s, dz, dgamma = ex.ls_case(B, N, Cc, form)
                assert (gamma is None) == (form in ("scale", "cast")) and (s is None) == (form in ("gamma", "cast"))
                assert torch.equal(g % 4, torch.zeros_like(g)) and torch.equal(dz, dz.round()) and dz.abs().max() <= 48 <= BF16_EXACT
                if s is not None:
                    seen |= set(s.tolist())
                if gamma is not None:
                    gs = g if s is None else g * s[:, None, None]
                    assert (gs.abs() * z.abs()).sum((0, 1)).max() + 100 < EXACT and z.abs().max() <= 3
                    naive = sum(gs[b, n] * z[b, n] for b in range(B) for n in range(min(N, 20))) if N <= 20 else None
                    assert naive is None or torch.equal(naive, dgamma)
    assert seen == set(ex.LS_SCALES)


# ------------------------------------------------------------------ 3. LayerNorm
def test_layernorm_tables():
    assert set(ex.LN_D) == {4, 32, 64, 68, 96, 128, 132, 160, 256, 260, 320, 512, 516, 768, 1024}
    assert {ex.ln_lanes(d) for d in ex.LN_D} == {(16, 1), (32, 1), (64, 1), (64, 2), (64, 4)}
    assert set(ex.LN_ROWS) == {1, 5, 6, 37, 300} and ex.LN_BIG == (8200, 32)
    assert ex.row_blocks(37) == 2 and ex.partition(300, 18) == (17, 18) and ex.partition(8200, 512)[1] == 483
    for D in ex.LN_D:
        for rows in (5, 37):
            x, gamma, beta, dy, dres = ex.ln_exact_operands(rows, D)
            assert torch.equal(x.abs(), torch.ones_like(x)) and (x.sum(1) == 0).all()
            ref = ex.ln_ref(x, gamma, beta, 0.0, dy, dres)
            assert torch.equal(ref["xhat"], x) and torch.equal(ref["y"], x * gamma + beta)          # rstd is exactly 1 in f64
            assert ref["y"].abs().max() <= 11 <= BF16_EXACT
            assert torch.equal(ref["dgamma"], ref["dgamma"].round()) and torch.equal(ref["dbeta"], dy.sum(0))
            if D & (D - 1) == 0:       # dx: multiples of 1/D, magnitude <= 3 * 6 + 2: 5 + 10 bits
                assert torch.equal(ref["dx"] * D, (ref["dx"] * D).round()) and ref["dx"].abs().max() <= 20
                assert torch.equal(ref["dx"].float().double(), ref["dx"])
    assert 2 * 8200 + 100 < EXACT and 6 * 1024 < EXACT               # dgamma / dbeta over 8200 rows; sum of g over a row


@pytest.mark.parametrize("kind", ex.LN_KINDS)
def test_layernorm_reference_matches_autograd(kind):
    rows, D = 5, 12
    x, gamma, beta, dy, dres = ex.ln_real_operands(rows, D, kind)
    dy = dy.double()
    ref = ex.ln_ref(x, gamma, beta, ex.LN_EPS, dy, dres)
    xr, g, b = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.layer_norm(xr, (D,), g, b, ex.LN_EPS)
    y.backward(dy)
    for key, t in (("y", y.detach()), ("dx", xr.grad + dres), ("dgamma", g.grad), ("dbeta", b.grad)):
        assert torch.allclose(ref[key], t, rtol=1e-9, atol=1e-9 * ref["s_" + key].max().item()), key
        assert (ref["s_" + key] >= ref[key].abs() * (1 - 1e-12)).all(), f"the scale of {key} is below the element itself"
    if kind.startswith("kappa"):
        k = x.mean(1).abs() / x.std(1, unbiased=False)
        assert ((k - float(kind[5:])).abs() <= 1e-3 * k).all(), "rows sit on their rung"
    if kind == "const3":
        assert torch.equal(ref["y"], beta.expand(rows, D))
    t32 = ex.ln_torch32(x, gamma, beta, ex.LN_EPS, dy, dres)
    assert all(t32[key].dtype == torch.float32 for key in t32)


# ------------------------------------------------------------------ 4. / 5. depthwise 3x3
def naive_dwconv(u, w9, bias):
    B, H, W, Cc = u.shape
    out = torch.zeros_like(u)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                acc = bias.clone()
                for r in range(3):
                    for s in range(3):
                        yy, xx = y + r - 1, x + s - 1
                        if 0 <= yy < H and 0 <= xx < W:
                            acc += u[b, yy, xx] * w9[3 * r + s]
                out[b, y, x] = acc
    return out


def test_dwconv_references_match_naive_loops():
    B, H, W, Cc = 2, 3, 4, 4
    u, w9, bias = ex.ints((B, H, W, Cc), 1, -3, 3), ex.ints((9, Cc), 2, -3, 3), ex.ints((Cc,), 3, -8, 8)
    ref = naive_dwconv(u, w9, bias)
    assert torch.equal(ex.ref_dwconv(u, w9, bias), ref) and ref.abs().max() > 8
    dpre = ex.ints((B, H, W, Cc), 4)
    dw, db = ex.ref_dw_bwd(u, dpre)
    wv = torch.zeros(9, Cc, dtype=torch.float64, requires_grad=True)
    bv = torch.zeros(Cc, dtype=torch.float64, requires_grad=True)
    ex.ref_dwconv(u, wv, bv).backward(dpre)
    assert torch.equal(dw, wv.grad) and torch.equal(db, bv.grad) and dw.abs().max() > 0


def test_dwconv_basis_shows_each_tap_at_its_neighbour():
    B, H, W, Cc = 1, 3, 70, 4
    w9, zero = ex.w9_basis(Cc), torch.zeros(Cc, dtype=torch.float64)
    for y0, x0 in ex.basis_pixels(H, W):
        u = torch.zeros(B, H, W, Cc, dtype=torch.float64)
        u[0, y0, x0] = 1.0
        out = ex.ref_dwconv(u, w9, zero)
        want = torch.zeros_like(out)
        for r in range(3):
            for s in range(3):
                y, x = y0 - (r - 1), x0 - (s - 1)
                if 0 <= y < H and 0 <= x < W:
                    want[0, y, x] = 3 * r + s + 1
        assert torch.equal(out, want)
        # backward: with dy one-hot, dw9[t] is the window at that pixel; with u one-hot, dw9[t] is dpre at the mirrored neighbour
        dense = ex.ints((B, H, W, Cc), 5, -3, 3)
        dw, db = ex.ref_dw_bwd(dense, u)
        assert torch.equal(dw, torch.stack([ex.shifted(dense, t // 3, t % 3)[0, y0, x0] for t in range(9)])) and (db == 1).all()
        dw, _ = ex.ref_dw_bwd(u, dense)
        assert torch.equal(dw, torch.stack([ex.shifted(dense, 2 - t // 3, 2 - t % 3)[0, y0, x0] for t in range(9)]))


def test_dwconv_forward_tables():
    assert {s[2] for s in ex.DW_DENSE} >= set(ex.DW_W) == {1, 2, 3, 4, 31, 32, 33, 34, 35, 64, 65, 70}
    assert {s[1] for s in ex.DW_DENSE} == set(ex.DW_H) and {s[0] for s in ex.DW_DENSE} == {1, 2}
    assert {s[3] for s in ex.DW_DENSE} >= set(ex.DW_C)
    tails = {W: (ex.segments(W)[-1][1] - ex.segments(W)[-1][0]) % 3 for W in ex.DW_W}
    assert tails == {1: 1, 2: 2, 3: 0, 4: 1, 31: 1, 32: 2, 33: 1, 34: 2, 35: 0, 64: 2, 65: 1, 70: 0}, "segment tail of 1, 2 or 0 mod 3"
    assert {len(ex.segments(W)) for W in ex.DW_W} == {1, 2, 3}
    for nb, shape in ex.DW_BLOCKS.items():
        assert ex.dw_fwd_blocks(*shape)[0] == nb, f"{nb} blocks"
    grids = {nb: ex.dw_fwd_blocks(*shape)[1] for nb, shape in ex.DW_BLOCKS.items()}
    assert grids == {1: 8, 7: 8, 8: 8, 9: 16, 17: 24}, "padded grid"
    for B, H, W, Cc in ex.DW_DENSE:                                  # |u| <= 3, |w| <= 3, |bias| <= 8: 81 + 8 within 2^8
        assert Cc % 4 == 0 and B * H * W * Cc * 4 <= 4 << 20
    assert 9 * 3 * 3 + 8 <= BF16_EXACT
    for B, H, W, Cc in ex.DW_BASIS:                                  # 9 taps x amplitudes 1..3
        px = ex.basis_pixels(H, W)
        assert (0, 0) in px and (H - 1, W - 1) in px and 9 * 3 <= BF16_EXACT
    px = ex.basis_pixels(3, 70)
    assert {x for _, x in px} == {0, 31, 32, 33, 63, 64, 69} and {y for y, _ in px} == {0, 2}, "both sides of each segment boundary"
    assert {x for _, x in ex.basis_pixels(2, 65)} == {0, 31, 32, 33, 63, 64} and {x for _, x in ex.basis_pixels(5, 34)} == {0, 31, 32, 33}


def test_dwconv_backward_tables():
    lanes, clamp = set(), set()
    for B, H, W, Cc in ex.DWB_SHAPES:
        nblk, rb, items = ex.dw_bwd_blocks(B, H, W, Cc)
        lanes.add(ex.dw_lanes(Cc))
        clamp.add(nblk < rb)
        assert 1 <= nblk <= rb and 2 * 3 * B * H * W + 100 < EXACT   # |dpre| <= 2, |u| <= 3 over every pixel, preset <= 100
    assert lanes == {16, 32, 64} and clamp == {True, False}, "the nblk clamp active and inactive"
    active = [s for s in ex.DWB_SHAPES if ex.dw_bwd_blocks(*s)[0] < ex.dw_bwd_blocks(*s)[1]]
    assert {ex.dw_lanes(s[3]) for s in active} == {16, 32, 64}
    assert any(ex.dw_bwd_blocks(*s)[0] > 1 for s in active), "more than one block of items"
    per, first_empty = ex.partition(ex.dw_bwd_blocks(2, 3, 70, 4)[2], ex.dw_bwd_blocks(2, 3, 70, 4)[0])
    assert (per, first_empty) == (9, 2)                              # 18 items in 2 blocks of 16 row slots: a ragged last pass
    assert {ex.dw_lanes(s[3]) for s in ex.DWB_BASIS} == {16, 32, 64}
    assert {(ex.segments(s[2])[-1][1] - ex.segments(s[2])[-1][0]) % 3 for s in ex.DWB_SHAPES} == {0, 1, 2}


# ------------------------------------------------------------------ 6. col2im
def naive_col2im(cols, B, Ho, Wo, k, Cc, stride, pad, H, W):
    dx = torch.zeros(B, H, W, Cc, dtype=torch.float64)
    c5 = cols.view(B, Ho, Wo, k * k, Cc)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for r in range(k):
                    for s in range(k):
                        y, x = oy * stride + r - pad, ox * stride + s - pad
                        if 0 <= y < H and 0 <= x < W:
                            dx[b, y, x] += c5[b, oy, ox, r * k + s]
    return dx


def test_col2im_table_and_reference():
    cases = ex.c2i_cases()
    assert {c[:3] for c in cases} == set(ex.C2I_GEOS) and {c[3:5] for c in cases} == set(ex.C2I_HW)
    assert {c[5] for c in cases} == {4, 32, 64} and {c[6] for c in cases} == {1, 2}
    dropped = [(g, hw) for g in ex.C2I_GEOS for hw in ex.C2I_HW if (*g, *hw) not in {c[:5] for c in cases}]
    assert all(g[0] > min(hw) + 2 * g[2] for g, hw in dropped), "only kernels larger than the padded map are left out"
    untouched = ragged = 0
    for k, stride, pad, H, W, Cc, B in cases:
        Ho, Wo = ex.conv_out(H, k, stride, pad), ex.conv_out(W, k, stride, pad)
        assert (-(-k // stride)) ** 2 * 2 <= BF16_EXACT               # taps on one pixel x |cols| <= 2
        cols = ex.ints((B * Ho * Wo, k * k * Cc), 100 * k + 10 * H + W + Cc)
        if H * W * Cc * B <= 3000:
            ref = ex.ref_col2im(cols, B, Ho, Wo, k, Cc, stride, pad, H, W)
            assert torch.equal(ref, naive_col2im(cols, B, Ho, Wo, k, Cc, stride, pad, H, W))
        ones = ex.ref_col2im(torch.ones_like(cols), B, Ho, Wo, k, Cc, stride, pad, H, W)
        untouched += bool((ones == 0).any())
        ragged += (H + 2 * pad - k) % stride != 0
    assert untouched >= 3 and ragged >= 3, "pixels that no tap touches; H not a multiple of the stride"
    ones = ex.ref_col2im(torch.ones(2 * 1, 16 * 4, dtype=torch.float64), 1, 2, 1, 4, 4, 4, 0, 9, 7)
    assert (ones[0, 8] == 0).all() and (ones[0, :8, 4:] == 0).all() and (ones[0, :8, :4] == 1).all()   # 9x7 under (4,4,0)


# ------------------------------------------------------------------ 7. softmax backward
def test_softmax_bwd_table():
    assert set(ex.SMB_COLS) == {1, 63, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048} and set(ex.SMB_ROWS) == {1, 5, 9}
    assert {min(-(-n // 64), 32) for n in ex.SMB_COLS} >= {1, 4, 5, 8, 9, 16, 17, 32}          # either side of every MAXV
    kinds = set()
    for n_cols in ex.SMB_COLS:
        assert n_cols in ex.smb_valid(n_cols) and (n_cols == 1 or min(ex.smb_valid(n_cols)) < n_cols)
        for rows in ex.SMB_ROWS:
            for n_valid in ex.smb_valid(n_cols):
                p, dp, ds, scale = ex.smb_case(rows, n_valid, n_cols, rows + n_valid + n_cols)
                assert p[:, n_valid:].isnan().all() and dp[:, n_valid:].isnan().all() and (ds[:, n_valid:] == 0).all()
                pv, dv = p[:, :n_valid], dp[:, :n_valid]
                assert torch.equal(pv.sum(1), torch.ones(rows, dtype=torch.float64))
                kinds |= {int((pv[r] != 0).sum()) for r in range(rows)}
                assert torch.equal(ds.bfloat16().double(), ds) and torch.equal(dv.bfloat16().double(), dv)
                assert scale in (0.125, 0.5, 1.0, 2.0)
                naive = torch.stack([pv[r] * (dv[r] - sum(pv[r, c] * dv[r, c] for c in pv[r].nonzero().flatten())) * scale
                                     for r in range(rows)])
                assert torch.equal(ds[:, :n_valid], naive)
    assert kinds == {1, 3}


# ------------------------------------------------------------------ 8. add_rows
def test_add_rows_table():
    assert any(a < rows and b is not None and b < rows and rows % a and rows % b for rows, a, b, D in ex.ADD_ROWS)
    assert any(b is None for _, _, b, _ in ex.ADD_ROWS) and any(rows * D > 256 * 256 for rows, _, _, D in ex.ADD_ROWS)
