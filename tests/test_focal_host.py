"""gdlhip.nn.FocalLoss, the parts that need no GPU: the reference formula the GPU tests hold the kernels against, the constructor
contract, the config alias and ``reads_lowres``.

Reference: smp 0.5.0 losses/focal.py + losses/_functional.py::focal_loss_with_logits restated in f64 (``focal_ref``).  smp itself
is not available, so parity with it is unpinned; what is pinned here is that torch autograd of the restatement equals the closed
form the kernels evaluate (``focal_grad_closed``), and that with ``gamma = 0`` and no ``alpha`` the loss is the sum over classes of
``BCEWithLogits`` taken over the valid pixels."""

import pytest
import torch
import torch.nn.functional as F

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402


def _z_and_valid(logits, target, mode, ignore_index):
    """(x, z, valid) broadcast to one entry per logit: z = [y == k] (multiclass) or [y == 1] (binary)."""
    if mode == "binary":
        x, t = logits.reshape(-1), target.reshape(-1)
        z = t == 1
        valid = torch.ones_like(z) if ignore_index is None else t != ignore_index
        return x, z.to(x.dtype), valid
    t = target[:, 0] if target.dim() == logits.dim() else target
    k = torch.arange(logits.shape[1]).view(1, -1, *([1] * (logits.dim() - 2)))
    z = t[:, None] == k
    valid = torch.ones_like(t, dtype=torch.bool) if ignore_index is None else t != ignore_index
    return logits, z.to(logits.dtype), valid[:, None].expand_as(z)


def _divisor(valid, logits, mode, reduction):
    if reduction == "sum":
        return 1.0
    n = valid.sum().item() if mode == "binary" else valid[:, 0].sum().item()
    return 1.0 / n if n > 0 else 0.0


def focal_ref(logits, target, mode="multiclass", alpha=None, gamma=2.0, ignore_index=None, reduction="mean", reduced_threshold=None):
    """smp's arithmetic in the dtype of ``logits``: BCE with logits, pt = exp(-BCE), the focal term from 1 - pt.  Without a valid
    pixel the result is 0 (the class's stated deviation)."""
    x, z, valid = _z_and_valid(logits, target, mode, ignore_index)
    logpt = F.binary_cross_entropy_with_logits(x, z, reduction="none")
    pt = torch.exp(-logpt)
    if reduced_threshold is None:
        focal = (1.0 - pt).pow(gamma)
    else:
        focal = ((1.0 - pt) / reduced_threshold).pow(gamma)
        focal = torch.where(pt < reduced_threshold, torch.ones_like(focal), focal)
    loss = focal * logpt
    if alpha is not None:
        loss = loss * (alpha * z + (1 - alpha) * (1 - z))
    total = torch.where(valid, loss, torch.zeros_like(loss)).sum()
    return total * _divisor(valid, logits, mode, reduction)


def focal_grad_closed(logits, target, mode="multiclass", alpha=None, gamma=2.0, ignore_index=None, reduction="mean",
                      reduced_threshold=None):
    """d focal_ref / d logits by the closed form -(2z - 1) a f (gamma pt L + q), in the dtype of ``logits``, every term from its
    own stable expression: finite for every gamma >= 0."""
    x, z, valid = _z_and_valid(logits, target, mode, ignore_index)
    s = (2 * z - 1) * x
    L, q, pt = F.softplus(-s), torch.sigmoid(-s), torch.sigmoid(s)
    g = torch.full_like(x, gamma)
    if reduced_threshold is None:
        f = torch.exp(-gamma * F.softplus(s))
    else:
        flat = pt < reduced_threshold
        f = torch.where(flat, torch.ones_like(x), torch.exp(-gamma * (F.softplus(s) + torch.log(torch.tensor(reduced_threshold, dtype=x.dtype)))))
        g = torch.where(flat, torch.zeros_like(g), g)
    a = 1.0 if alpha is None else alpha * z + (1 - alpha) * (1 - z)
    grad = -(2 * z - 1) * a * f * (g * pt * L + q)
    grad = torch.where(valid, grad, torch.zeros_like(grad)) * _divisor(valid, logits, mode, reduction)
    return grad.reshape(logits.shape)


def threshold_margin(logits, target, th, **kw):
    """min |pt - th| over the elements of the f64 reference (the loss and its gradient jump at pt == th)."""
    x, z, _ = _z_and_valid(logits.double(), target, kw.get("mode", "multiclass"), None)
    return (torch.sigmoid((2 * z - 1) * x) - th).abs().min().item()


def nudge_off_threshold(logits, target, th, margin=1e-4, mode="multiclass"):
    """``logits`` (f32) with every element whose pt lies within ``margin`` of ``th`` pushed 0.02 in s away from the switch;
    returns (logits, number of elements moved)."""
    x, z, _ = _z_and_valid(logits.double(), target, mode, None)
    sign = 2 * z - 1
    s = sign * x
    near = (torch.sigmoid(s) - th).abs() < margin
    s0 = torch.logit(torch.tensor(th, dtype=torch.float64))
    moved = torch.where(s >= s0, s0 + 0.02, s0 - 0.02)
    out = torch.where(near, sign * moved, x).reshape(logits.shape).float()
    return out, int(near.sum().item())


def _data(K, seed=0, ignore=None, shape=(2, 13, 11), scale=3.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape[0], K, *shape[1:], generator=g) * scale).double()
    y = torch.randint(0, K, shape, generator=g)
    if ignore is not None:
        y[torch.rand(shape, generator=g) < 0.2] = ignore
    return x, y


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("th", [None, 0.3, 0.5])
@pytest.mark.parametrize("ignore", [None, 255])
@pytest.mark.parametrize("alpha", [None, 0.25, 0.75])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0])
def test_autograd_of_the_restatement_equals_the_closed_form(gamma, alpha, ignore, th, reduction):
    """randn * 3 in f64 keeps q = 1 - pt away from 0, where torch's pow has no gradient for gamma = 0.5: both exist here."""
    for K in (2, 5):
        x, y = _data(K, seed=K, ignore=ignore)
        kw = dict(alpha=alpha, gamma=gamma, ignore_index=ignore, reduction=reduction, reduced_threshold=th)
        if th is not None:
            assert threshold_margin(x, y, th) > 1e-9
        a = x.clone().requires_grad_(True)
        focal_ref(a, y, **kw).backward()
        closed = focal_grad_closed(x, y, **kw)
        assert torch.isfinite(a.grad).all()
        assert (a.grad - closed).abs().max().item() <= 1e-12 * max(1.0, closed.abs().max().item())


def test_binary_reference_and_closed_form():
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(2, 1, 9, 7, generator=g) * 3).double()
    y = torch.randint(0, 2, (2, 9, 7), generator=g)
    y[torch.rand(y.shape, generator=g) < 0.2] = 255
    y[0, 0, :3] = 7          # neither 1 nor ignore_index: a negative
    kw = dict(mode="binary", alpha=0.25, gamma=2.0, ignore_index=255)
    a = x.clone().requires_grad_(True)
    loss = focal_ref(a, y, **kw)
    loss.backward()
    assert (a.grad - focal_grad_closed(x, y, **kw)).abs().max().item() <= 1e-14
    as_zero = y.clone()
    as_zero[0, 0, :3] = 0
    assert loss.item() == focal_ref(x, as_zero, **kw).item()
    assert (a.grad.reshape(2, 9, 7)[y == 255] == 0).all()


@pytest.mark.parametrize("ignore", [None, 255])
def test_without_focusing_and_alpha_it_is_bce_with_logits_summed_over_classes(ignore):
    x, y = _data(5, seed=3, ignore=ignore)
    valid = torch.ones_like(y, dtype=torch.bool) if ignore is None else y != ignore
    want = sum(F.binary_cross_entropy_with_logits(x[:, k][valid], (y == k)[valid].double()) for k in range(5))
    got = focal_ref(x, y, gamma=0.0, ignore_index=ignore)
    assert abs(got.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))


def test_reference_out_of_range_target_is_a_valid_all_negative_pixel_and_no_valid_pixel_gives_zero():
    x, y = _data(4, seed=4)
    bad = y.clone()
    bad[0, :2] = 4
    bad[0, 2] = -3
    bad[0, 3] = 2**33 + 1
    z, _ = F.one_hot(y, 4).permute(0, 3, 1, 2).double(), None
    z[0, :, :4] = 0
    L = F.binary_cross_entropy_with_logits(x, z, reduction="none")
    want = ((1 - torch.exp(-L)) ** 2 * L).sum() / y.numel()
    assert abs(focal_ref(x, bad).item() - want.item()) <= 1e-12
    none = torch.full_like(y, 255)
    a = x.clone().requires_grad_(True)
    loss = focal_ref(a, none, ignore_index=255)
    loss.backward()
    assert loss.item() == 0.0 and (a.grad == 0).all() and (focal_grad_closed(x, none, ignore_index=255) == 0).all()


def test_closed_form_is_finite_where_autograd_is_not():
    """Logits of +-80 at gamma 0.5: q is exactly 0 in f64 for the confident elements and torch's pow backward gives NaN there."""
    g = torch.Generator().manual_seed(5)
    x = ((torch.randint(0, 2, (2, 5, 7, 6), generator=g).double() * 2 - 1) * 80.0)
    y = torch.randint(0, 5, (2, 7, 6), generator=g)
    a = x.clone().requires_grad_(True)
    focal_ref(a, y, gamma=0.5).backward()
    assert torch.isnan(a.grad).any()
    closed = focal_grad_closed(x, y, gamma=0.5)
    assert torch.isfinite(closed).all() and closed.abs().max().item() > 0


@pytest.mark.parametrize("th", [0.5, 0.3])
def test_threshold_nudges_are_a_handful(th):
    """The shapes and seeds tests/test_hip_focal.py::test_reduced_threshold uses: few elements sit within 1e-4 of pt == th, and
    after the nudge none does."""
    for K in (2, 5):
        g = torch.Generator().manual_seed(K)
        x = torch.randn(2, K, 37, 41, generator=g) * 2
        y = torch.randint(0, K, (2, 37, 41), generator=g)
        moved, n = nudge_off_threshold(x, y, th)
        print(f"K={K} th={th}: {n} of {x.numel()} elements nudged, margin afterwards {threshold_margin(moved, y, th):.2e}")
        assert n <= 8
        assert threshold_margin(moved, y, th) >= 1e-4
        assert (moved != x).sum().item() <= n


# ------------------------------------------------------------------------------------------------ the class
def test_constructor_accepts_smp_arguments_and_rejects_the_rest():
    crit = gnn.FocalLoss("multiclass")
    assert (crit.mode, crit.alpha, crit.gamma, crit.ignore_index, crit.reduction, crit.normalized, crit.reduced_threshold) == \
        ("multiclass", None, 2.0, None, "mean", False, None)
    assert crit.options == ops.FocalOptions(2.0, None, None, True, None)
    assert crit.options.c_args() == (2.0, 0, 0.0, 0, 0.0, 0, 0, 1)
    crit = gnn.FocalLoss("binary", alpha=0.25, gamma=0.5, ignore_index=255, reduction="sum", reduced_threshold=0.3)
    assert crit.options == ops.FocalOptions(0.5, 0.25, 255, False, 0.3)
    assert crit.options.c_args() == (0.5, 1, 0.25, 1, 0.3, 1, 255, 0)
    assert gnn.FocalLoss("multiclass", gamma=0, alpha=0.0, ignore_index=-1, reduced_threshold=1.0).options.c_args() == \
        (0.0, 1, 0.0, 1, 1.0, 1, -1, 1)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gamma"):
            gnn.FocalLoss("multiclass", gamma=bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            gnn.FocalLoss("multiclass", alpha=bad)
    for bad in (0.0, -0.2, 1.01, float("nan")):
        with pytest.raises(ValueError, match="reduced_threshold"):
            gnn.FocalLoss("multiclass", reduced_threshold=bad)
    for bad in (2.5, True, 2**63):
        with pytest.raises(ValueError, match="ignore_index"):
            gnn.FocalLoss("multiclass", ignore_index=bad)
    with pytest.raises(ValueError, match="reduction"):
        gnn.FocalLoss("multiclass", reduction="median")
    with pytest.raises(ValueError, match="mode"):
        gnn.FocalLoss("regression")


@pytest.mark.parametrize("kw", [dict(normalized=True), dict(reduction="none"), dict(reduction="batchwise_mean"), dict(mode="multilabel")])
def test_unimplemented_arguments_raise_and_name_what_is_implemented(kw):
    with pytest.raises(NotImplementedError, match="implements"):
        gnn.FocalLoss(**{"mode": "multiclass", **kw})


def test_reads_lowres_for_both_modes():
    assert gnn.reads_lowres(gnn.FocalLoss("multiclass", alpha=0.25))
    assert not gnn.reads_lowres(gnn.FocalLoss("binary"))


def test_config_alias_resolves_to_the_hip_loss():
    from geo_deep_learning import train as gdl_train
    crit = gdl_train.instantiate({"class_path": "segmentation_models_pytorch.losses.FocalLoss",
                                  "init_args": {"mode": "multiclass", "alpha": 0.25}})
    assert type(crit) is gnn.FocalLoss and crit.options == ops.FocalOptions(2.0, 0.25, None, True, None)


def test_ops_refuse_cpu_tensors():
    x, y = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    low, up, norm = torch.zeros(1, 2, 2, 3), torch.ones(()), torch.ones(1)
    for call in (lambda: ops.focal_fwd(x, y), lambda: ops.focal_bwd(x, y, norm, up),
                 lambda: ops.focal_binary_fwd(x[:, :1], y), lambda: ops.focal_binary_bwd(x[:, :1], y, norm, up),
                 lambda: ops.focal_lowres_fwd(low, y, (4, 4)), lambda: ops.focal_lowres_bwd(low, y, (4, 4), norm, up),
                 lambda: gnn.FocalLoss("multiclass")(x, y), lambda: gnn.FocalLoss("binary")(x[:, :1], y)):
        with pytest.raises(ValueError):
            call()
    assert not ops.focal_lowres_ok(torch.zeros(1, 12, 12, 5), (8, 8)) and ops.focal_lowres_ok(low, (4, 4))
