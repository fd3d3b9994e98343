"""The integer reference of tests/test_hip_wgrad_exact.py, tested where there is no GPU: against a naive loop over pixels,
taps and channels on a 2 x 3 x 3 example, and the 2^24 bound that makes the comparison exact."""

import pytest
import torch

import test_hip_wgrad_exact as ex


def naive_wgrad(x, dy, R, S, stride, pad):
    B, H, W, Cc = x.shape
    _, Ho, Wo, N = dy.shape
    dw = torch.zeros(N, R * S * Cc, dtype=torch.int64)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for r in range(R):
                    for s in range(S):
                        iy, ix = oy * stride + r - pad, ox * stride + s - pad
                        if 0 <= iy < H and 0 <= ix < W:
                            for n in range(N):
                                for c in range(Cc):
                                    dw[n, (r * S + s) * Cc + c] += int(dy[b, oy, ox, n]) * int(x[b, iy, ix, c])
    return dw.float()


@pytest.mark.parametrize("R,S,stride,pad", [(1, 1, 1, 0), (3, 3, 1, 1), (3, 3, 2, 1), (2, 2, 2, 0), (3, 1, 1, 1), (1, 3, 1, 1)])
def test_integer_reference_matches_naive_loops(R, S, stride, pad):
    B, H, W, Cc, N = 2, 3, 3, 3, 2
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    x, dy = ex.ints((B, H, W, Cc), 1), ex.ints((B, Ho, Wo, N), 2)
    want = naive_wgrad(x, dy, R, S, stride, pad)
    assert want.abs().max() > 0
    assert torch.equal(ex.ref_conv_wgrad(x, dy, R, S, stride, pad), want)
    if (R, S, stride, pad) == (1, 1, 1, 0):
        assert torch.equal(ex.ref_gemm_wgrad(x.reshape(-1, Cc), dy.reshape(-1, N)), want)
        x3, dy3 = torch.stack([x, 2 * x]).reshape(2, -1, Cc), torch.stack([dy, dy]).reshape(2, -1, N)
        assert torch.equal(ex.ref_gemm_wgrad(x3, dy3), torch.stack([want, 2 * want]))


def test_grouped_integer_reference_matches_naive_loops():
    x, dy = ex.ints((2, 3, 3, 4), 3), ex.ints((2, 3, 3, 6), 4)
    got = ex.ref_conv_wgrad(x, dy, 3, 3, 1, 1, groups=2)
    for z in range(2):
        assert torch.equal(got[3 * z:3 * z + 3], naive_wgrad(x[..., 2 * z:2 * z + 2], dy[..., 3 * z:3 * z + 3], 3, 3, 1, 1))


def test_ints_is_seeded_and_bounded():
    a, b = ex.ints((4, 5), 7), ex.ints((4, 5), 7)
    assert torch.equal(a, b) and not torch.equal(a, ex.ints((4, 5), 8))
    t = ex.ints((1000,), 0, -3, 1)
    assert t.min() == -3 and t.max() == 1 and torch.equal(t, t.round())


def test_exact_bound():
    x, dy = torch.full((4,), 2.0, dtype=torch.float64), torch.full((4,), -2.0, dtype=torch.float64)
    assert ex.assert_exact_bound(x, dy, 1000) == 4000
    assert ex.assert_exact_bound(x, dy, (1 << 22) - 1, torch.tensor([3.0], dtype=torch.float64)) == (1 << 24) - 1
    with pytest.raises(AssertionError):
        ex.assert_exact_bound(x, dy, 1 << 22)                      # 4 P = 2^24: the largest partial sum may round
    with pytest.raises(AssertionError):
        ex.assert_exact_bound(x, dy, (1 << 22) - 1, torch.tensor([-4.0], dtype=torch.float64))
    with pytest.raises(AssertionError):
        ex.assert_exact_bound(x * 0.75, dy, 10)                    # not integers


def test_last_split_arithmetic():
    """The issue's example: P = 6150 in 12 bf16 splits of 576 pixels leaves the twelfth empty."""
    a = ex._lib.WgradArgs()
    a.dtype, a.B, a.Ho, a.Wo, a.H, a.W = ex.ops.BF16, 1, 1, 6150, 1, 6150
    assert ex.last_split(a, 12, "tr128") == "empty" and ex.last_split(a, 11, "tr128") == "ragged"
    a.Wo = 8 * 576 + 3
    assert ex.last_split(a, 9, "tr128") == "short"
    a.B, a.H, a.W = 3, 27, 32
    assert ex.last_split(a, 10, "rows") == "empty" and ex.last_split(a, 9, "rows") == "full"
