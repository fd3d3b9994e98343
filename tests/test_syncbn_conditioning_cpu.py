"""CPU twin of tests/test_hip_bn_conditioning.py::test_syncbn_merge_ladder for the torch-expression fallback of
gdlhip.nn.sync_batch_stats (sync_message / sync_message_stats): the count-weighted SyncBatchNorm merge of three "ranks" with
unequal pixel counts on the kappa = |mean| / std ladder, without a process group (a torch add stands for the all-reduce),
against the f64 statistics of the concatenation.  Bounds as in the GPU module: variance 1e-5 (v + eps), mean 2 f32 ulps + 1e-6 std."""

import pytest
import torch

from gdlhip import nn as gnn

EPS = 1e-5
RANK_PIXELS = (126, 63, 9)


def ulp32(t):
    a = t.abs().float().clamp_min(1e-38)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def ranks(rung, std, C=64, exact_means=True):
    """local (mean, var, count) in f32 of three ranks whose means differ by up to 5 std, the f64 statistics of all their pixels, a
    pivot within a few std of the global mean (the layer's running_mean: identical on every rank), and what rounding the rank
    means to f32 alone moves the merged variance by (0 when ``exact_means`` makes them f32 numbers beforehand)"""
    g = torch.Generator().manual_seed(1000 + int(rung * 4) + int(std * 100))
    parts = [(torch.randn(n, C, generator=g, dtype=torch.float64) + 2 * rung + s) * std for n, s in zip(RANK_PIXELS, (0.0, 3.0, -2.0))]
    # each rank's mean is an f32 number: rounding it would move the between-rank variance before any merge runs
    if exact_means:
        parts = [p + (p.mean(0).float().double() - p.mean(0)) for p in parts]
    full = torch.cat(parts)
    m, v = full.mean(0), full.var(0, unbiased=False)
    local = [(p.mean(0).float(), p.var(0, unbiased=False).float(), float(p.shape[0])) for p in parts]
    pivot = (m + 2.0 * std * torch.randn(C, generator=g, dtype=torch.float64)).float()
    # first order of the between-rank part sum_r n_r / n (mean_r - mean)^2 under half an ulp of each mean_r
    term = sum(p.shape[0] / full.shape[0] * (p.mean(0) - m).abs() * ulp32(p.mean(0)) for p in parts)
    return local, m, v, pivot, (0.0 if exact_means else term)


def merge(local, pivot):
    C = local[0][0].numel()
    packed = sum(torch.cat(gnn.sync_message(mean, var, n, pivot)) for mean, var, n in local)
    return gnn.sync_message_stats(packed, C, pivot)


@pytest.mark.parametrize("exact_means", [True, False])
@pytest.mark.parametrize("std", [1.0, 0.01])
@pytest.mark.parametrize("rung", [0.25, 30.0, 300.0, 1000.0])
def test_syncbn_fallback_merge_ladder(rung, std, exact_means):
    """exact_means: the merge arithmetic alone.  Otherwise the rank means are rounded to f32 as bn_stats hands them over, and the
    bound carries that input rounding (2e-5 of the variance at kappa = 300 with rank means 5 std apart)."""
    local, m, v, pivot, term = ranks(rung, std, exact_means=exact_means)
    kappa = m.abs() / v.sqrt()
    assert (kappa >= 0.9 * rung).double().mean().item() >= 0.75, kappa.median().item()
    gmean, gvar, total = merge(local, pivot)
    assert float(total) == float(sum(RANK_PIXELS))
    raw = ((gvar.double() - v).abs() / (v + EPS)).max().item()
    ev = (((gvar.double() - v).abs() - term).clamp_min(0) / (v + EPS)).max().item()
    em = ((gmean.double() - m).abs() / (2 * ulp32(m) + 1e-6 * v.sqrt())).max().item()
    # the plain message (pivot 0: layers without running buffers) on the same ranks, for the record
    _, pvar, _ = merge(local, None)
    print(f"BNCOND syncbn fallback rung={rung:g} std={std:g} kappa={kappa.median().item():.4g} {'exact' if exact_means else 'rounded'} rank means var_err={raw:.3e} beyond input rounding={ev:.3e} mean_err/tol={em:.3f} "
          f"(pivot 0: var_err={((pvar.double() - v).abs() / (v + EPS)).max().item():.3e})")
    assert ev <= 1e-5 and em <= 1.0


def test_syncbn_fallback_without_pivot_is_the_plain_message():
    """no running buffers -> pivot 0: [n mean | n (var + mean^2) | n], exact to round-off on a tame layer"""
    local, m, v, _, _ = ranks(0.25, 1.0)
    mean, var, n = local[0]
    a, b, c = gnn.sync_message(mean, var, n)
    assert torch.equal(a, mean * n) and torch.equal(b, (var + mean * mean) * n) and c.item() == n
    gmean, gvar, _ = merge(local, None)
    assert ((gvar.double() - v).abs() / (v + EPS)).max().item() <= 1e-5
    assert ((gmean.double() - m).abs() <= 2 * ulp32(m) + 1e-6 * v.sqrt()).all()


def test_sync_pivot_pads_the_running_mean_to_the_padded_channel_count():
    rm = torch.arange(5, dtype=torch.float32)
    assert gnn._sync_pivot(None, 8) is None
    assert gnn._sync_pivot(rm, 5).data_ptr() == rm.data_ptr()
    assert torch.equal(gnn._sync_pivot(rm, 8), torch.tensor([0., 1., 2., 3., 4., 0., 0., 0.]))
