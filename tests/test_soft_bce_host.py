"""gdlhip.nn.SoftBCEWithLogitsLoss, the parts that need no GPU: the reference formula the GPU tests hold the kernels against, the
constructor contract, the state-dict keys, the config alias and ``reads_lowres``.

Reference: smp 0.5.0 losses/soft_bce.py restated in f64.  ``soft_bce_ref`` writes the closed form out -- it does not call
``F.binary_cross_entropy_with_logits`` -- and is pinned here against smp's forward restated with torch's own
``F.binary_cross_entropy_with_logits`` (``smp_forward``) to 1e-12 relative, and its autograd gradient against the closed form
``dl/dx`` (``soft_bce_grad_closed``).  smp itself is not available, so parity with it is unpinned."""

import itertools

import pytest
import torch
import torch.nn.functional as F

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402


def _terms(x, y, weight, pos_weight, smooth_factor, ignore_index):
    """(x, t, w, p, valid) in f64, one entry per logit: the smoothed target, the broadcast weights and the ignore mask, which is
    taken from the RAW target in its own dtype."""
    x = x.double()
    raw = y.reshape(x.shape)
    valid = torch.ones_like(raw, dtype=torch.bool) if ignore_index is None else raw != ignore_index
    yv = raw.double()
    t = yv if smooth_factor is None else (1 - yv) * smooth_factor + yv * (1 - smooth_factor)
    w = torch.ones((), dtype=torch.float64) if weight is None else weight.double()
    p = torch.ones((), dtype=torch.float64) if pos_weight is None else pos_weight.double()
    return x, t, w, p, valid


def soft_bce_ref(x, y, *, weight=None, pos_weight=None, smooth_factor=None, ignore_index=-100, reduction="mean"):
    """l = w ((1 - t) x + (1 + (p - 1) t) softplus(-x)), softplus(-x) = max(-x, 0) + log1p(exp(-|x|)), selected by
    y != ignore_index and reduced over ALL elements ("mean": the divisor counts the ignored ones) in f64."""
    x, t, w, p, valid = _terms(x, y, weight, pos_weight, smooth_factor, ignore_index)
    softplus_neg = torch.clamp(-x, min=0) + torch.log1p(torch.exp(-x.abs()))
    l = w * ((1 - t) * x + (1 + (p - 1) * t) * softplus_neg)
    l = torch.where(valid, l, torch.zeros_like(l))
    return l.mean() if reduction == "mean" else l.sum()


def soft_bce_grad_closed(x, y, *, weight=None, pos_weight=None, smooth_factor=None, ignore_index=-100, reduction="mean"):
    """d soft_bce_ref / dx by the closed form w ((1 - t) - (1 + (p - 1) t) sigmoid(-x)), sigmoid(-x) from e = exp(-|x|)."""
    x, t, w, p, valid = _terms(x, y, weight, pos_weight, smooth_factor, ignore_index)
    e = torch.exp(-x.abs())
    sig_neg = torch.where(x >= 0, e / (1 + e), 1 / (1 + e))
    g = (w * ((1 - t) - (1 + (p - 1) * t) * sig_neg)).expand_as(x)
    g = torch.where(valid, g, torch.zeros_like(g))
    return g / x.numel() if reduction == "mean" else g


def smp_forward(x, y, *, weight=None, pos_weight=None, smooth_factor=None, ignore_index=-100, reduction="mean"):
    """smp's forward, line by line, on f64 tensors with torch's own binary_cross_entropy_with_logits."""
    x = x.double()
    y_true = y.reshape(x.shape)
    yv = y_true.double()
    soft = (1 - yv) * smooth_factor + yv * (1 - smooth_factor) if smooth_factor is not None else yv
    loss = F.binary_cross_entropy_with_logits(x, soft, None if weight is None else weight.double(),
                                              pos_weight=None if pos_weight is None else pos_weight.double(), reduction="none")
    if ignore_index is not None:
        loss = loss * (y_true != ignore_index)
    return loss.mean() if reduction == "mean" else loss.sum()


# the option grid (shared with tests/test_hip_soft_bce.py): smoothing, per-channel weights, ignore_index, reduction
GRID = [dict(smooth_factor=s, per_channel=pc, ignore_index=ig, reduction=r)
        for s, pc, ig, r in itertools.product((None, 0.1), (False, True), (None, -100, 255), ("mean", "sum"))]


def grid_id(o):
    return f"s{o['smooth_factor']}-{'wp' if o['per_channel'] else 'nowp'}-ig{o['ignore_index']}-{o['reduction']}"


def channel_weights(C, shape4=False):
    """Per-channel ``weight`` [C,1,1] and ``pos_weight`` [C,1,1] (or [1,C,1,1]), all different, f32."""
    w = (0.5 + 0.25 * torch.arange(C, dtype=torch.float32)).view(C, 1, 1)
    p = (2.0 - 0.5 * torch.arange(C, dtype=torch.float32)).clamp(min=0.25).view(C, 1, 1)
    return (w[None], p[None]) if shape4 else (w, p)


def make_case(shape, float_target, ignore_index, seed=0, scale=3.0, extreme=50.0):
    """f32 logits [B,C,H,W] (randn * scale, about one in eight set to +-extreme) and a target of the same numel: int64 0/1 shaped
    [B,H,W] where C == 1, or f32 with fractional values; with ``ignore_index`` about 15 % of it holds that value."""
    g = torch.Generator().manual_seed(seed + sum(shape))
    x = torch.randn(shape, generator=g) * scale
    if extreme:
        hit = torch.rand(shape, generator=g) < 0.125
        sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
        x = torch.where(hit, sign * extreme, x)
    tshape = (shape[0], *shape[2:]) if shape[1] == 1 and not float_target else shape
    y = torch.rand(tshape, generator=g) if float_target else torch.randint(0, 2, tshape, generator=g)
    if ignore_index is not None:
        y[torch.rand(tshape, generator=g) < 0.15] = ignore_index
    return x, y


def options_of(o, C):
    """The keyword arguments of soft_bce_ref / the class for a GRID entry on C channels."""
    w, p = channel_weights(C) if o["per_channel"] else (None, None)
    return dict(weight=w, pos_weight=p, smooth_factor=o["smooth_factor"], ignore_index=o["ignore_index"], reduction=o["reduction"])


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("float_target", [False, True], ids=["int64", "f32"])
@pytest.mark.parametrize("o", GRID, ids=grid_id)
def test_the_closed_form_is_smp_forward_and_its_gradient(o, float_target):
    for shape in ((2, 3, 7, 5), (2, 1, 9, 4)):
        kw = options_of(o, shape[1])
        x, y = make_case(shape, float_target, o["ignore_index"], seed=3)
        assert (x == 50).any() and (x == -50).any()
        if o["ignore_index"] is not None:
            assert 2 <= (y == o["ignore_index"]).sum().item() < y.numel() // 2
        a = x.double().requires_grad_(True)
        ref = soft_bce_ref(a, y, **kw)
        want = smp_forward(x, y, **kw)
        assert torch.isfinite(ref).item() and ref.item() > 0
        assert abs(ref.item() - want.item()) <= 1e-12 * abs(want.item()), (ref.item(), want.item())
        ref.backward()
        closed = soft_bce_grad_closed(x, y, **kw)
        assert torch.isfinite(a.grad).all()
        assert (a.grad - closed).abs().max().item() <= 1e-12 * closed.abs().max().item()
        if o["ignore_index"] is not None:
            assert (a.grad[y.reshape(x.shape) == o["ignore_index"]] == 0).all()


def test_mean_divides_by_every_element_and_the_ignore_test_precedes_smoothing():
    x = torch.tensor([[[[0.5, -1.0, 2.0, 0.0]]]])
    y = torch.tensor([[[1, 0, 255, 255]]])
    got = soft_bce_ref(x, y, ignore_index=255, smooth_factor=0.2)
    t = torch.tensor([0.8, 0.2], dtype=torch.float64)
    two = F.binary_cross_entropy_with_logits(x.double().reshape(-1)[:2], t, reduction="sum")
    assert abs(got.item() - two.item() / 4) <= 1e-15
    # a float target equal to ignore_index is ignored as a float compare; 254.5 is a (strange but legal) target value
    yf = torch.tensor([[[[1.0, 0.25, 255.0, 254.5]]]])
    a = soft_bce_ref(x, yf, ignore_index=255, reduction="sum")
    b = F.binary_cross_entropy_with_logits(x.double().reshape(-1)[[0, 1, 3]], yf.double().reshape(-1)[[0, 1, 3]], reduction="sum")
    assert abs(a.item() - b.item()) <= 1e-12 * abs(b.item())


def test_a_non_finite_logit_under_an_ignored_pixel_does_not_poison_the_reference():
    x = torch.tensor([[[[0.5, float("nan"), float("inf")]]]])
    y = torch.tensor([[[1, 255, 255]]])
    loss = soft_bce_ref(x, y, ignore_index=255, reduction="sum")
    assert abs(loss.item() - F.softplus(torch.tensor(-0.5, dtype=torch.float64)).item()) <= 1e-15
    closed = soft_bce_grad_closed(x, y, ignore_index=255, reduction="sum")
    assert torch.isfinite(closed).all() and (closed.reshape(-1)[1:] == 0).all()


# ------------------------------------------------------------------------------------------------ the class
def test_constructor_has_smp_signature_and_defaults():
    crit = gnn.SoftBCEWithLogitsLoss()
    assert (crit.weight, crit.ignore_index, crit.reduction, crit.smooth_factor, crit.pos_weight) == (None, -100, "mean", None, None)
    assert crit._options() == ops.SoftBCEOptions(None, -100, True, None, None)
    assert crit._options().c_args(8)[:5] == (0, 0.0, 1, -100, -100.0) and crit._options().c_args(8)[5:] == (None, 0, None, 0, 0.125)
    w, p = channel_weights(3)
    crit = gnn.SoftBCEWithLogitsLoss(w, None, "sum", 0.1, p)
    o = crit._options()
    assert (o.smooth_factor, o.ignore_index, o.mean) == (0.1, None, False) and torch.equal(o.weight, w) and torch.equal(o.pos_weight, p)
    assert o.c_args(8)[:5] == (1, 0.1, 0, 0, 0.0) and o.c_args(8)[6::2] == (3, 3) and o.c_args(8)[9] == 1.0
    crit = gnn.SoftBCEWithLogitsLoss(weight=torch.tensor(2.0), pos_weight=channel_weights(4, shape4=True)[1], ignore_index=255,
                                     smooth_factor=0)
    assert crit.weight.numel() == 1 and crit.pos_weight.shape == (1, 4, 1, 1) and crit.smooth_factor == 0.0


def test_constructor_rejects_what_the_issue_lists():
    with pytest.raises(NotImplementedError, match="implements"):
        gnn.SoftBCEWithLogitsLoss(reduction="none")
    for bad in ("median", "batchwise_mean", None):
        with pytest.raises(ValueError, match="reduction"):
            gnn.SoftBCEWithLogitsLoss(reduction=bad)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="smooth_factor"):
            gnn.SoftBCEWithLogitsLoss(smooth_factor=bad)
    for bad in (2.5, True, 2**63):
        with pytest.raises(ValueError, match="ignore_index"):
            gnn.SoftBCEWithLogitsLoss(ignore_index=bad)
    # anything that broadcasts against [B,C,H,W] but varies over more than the channel dimension
    for shape in ((3,), (5, 7), (1, 7), (3, 1, 7), (2, 3, 1, 1), (3, 5, 7)):
        for name in ("weight", "pos_weight"):
            with pytest.raises(NotImplementedError, match="implements"):
                gnn.SoftBCEWithLogitsLoss(**{name: torch.ones(shape)})


def test_state_dict_keys_are_smps():
    w, p = channel_weights(3)
    crit = gnn.SoftBCEWithLogitsLoss(weight=w, pos_weight=p)
    sd = crit.state_dict()
    assert list(sd) == ["weight", "pos_weight"] and torch.equal(sd["weight"], w) and torch.equal(sd["pos_weight"], p)
    assert list(gnn.SoftBCEWithLogitsLoss().state_dict()) == []
    other = gnn.SoftBCEWithLogitsLoss(weight=torch.zeros(3, 1, 1), pos_weight=torch.zeros(3, 1, 1))
    other.load_state_dict(sd)
    assert torch.equal(other.weight, w) and torch.equal(other._options().pos_weight, p)


def test_reads_lowres_for_one_class_only_and_unchanged_for_the_other_losses():
    crit = gnn.SoftBCEWithLogitsLoss()
    assert gnn.reads_lowres(crit, 1) and not gnn.reads_lowres(crit, 2) and not gnn.reads_lowres(crit) and not gnn.reads_lowres(crit, 5)
    for cls in (gnn.DiceLoss, gnn.JaccardLoss, gnn.TverskyLoss, gnn.FocalLoss):
        assert gnn.reads_lowres(cls("multiclass")) and gnn.reads_lowres(cls("multiclass"), 1) and gnn.reads_lowres(cls("multiclass"), 5)
        assert gnn.reads_lowres(cls("binary"), 1) and not gnn.reads_lowres(cls("binary"), 2) and not gnn.reads_lowres(cls("binary"))
    for n in (None, 1, 5):
        assert gnn.reads_lowres(gnn.SoftCrossEntropyLoss(smooth_factor=0.1), n)
        assert not gnn.reads_lowres(gnn.LovaszLoss("multiclass"), n) and not gnn.reads_lowres(gnn.LovaszLoss("binary"), n)
        assert not gnn.reads_lowres(torch.nn.BCEWithLogitsLoss(), n) and not gnn.reads_lowres(torch.nn.CrossEntropyLoss(), n)


def test_config_alias_resolves_to_the_hip_loss():
    from geo_deep_learning import train as gdl_train
    crit = gdl_train.instantiate({"class_path": "segmentation_models_pytorch.losses.SoftBCEWithLogitsLoss",
                                  "init_args": {"smooth_factor": 0.1, "ignore_index": 255}})
    assert type(crit) is gnn.SoftBCEWithLogitsLoss and (crit.smooth_factor, crit.ignore_index, crit.reduction) == (0.1, 255, "mean")
    assert "torch.nn.BCEWithLogitsLoss" not in gdl_train.CLASS_ALIASES
    assert "SoftBCEWithLogitsLoss" in gdl_train.__doc__


def test_ops_and_class_refuse_cpu_tensors():
    x, y = torch.zeros(1, 1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    low, up = torch.zeros(1, 2, 2, 1), torch.ones(())
    for call in (lambda: ops.soft_bce_fwd(x, y), lambda: ops.soft_bce_bwd(x, y, up),
                 lambda: ops.soft_bce_lowres_fwd(low, y, (4, 4)), lambda: ops.soft_bce_lowres_bwd(low, y, (4, 4), up),
                 lambda: gnn.SoftBCEWithLogitsLoss()(x, y), lambda: gnn.SoftBCEWithLogitsLoss()(x, y.float())):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="do not match"):
        gnn.SoftBCEWithLogitsLoss()(x, torch.zeros(1, 4, 5))
