"""gdlhip.nn.CrossEntropyLoss, the parts that need no GPU: the reference formula the GPU tests hold the kernels against, the
constructor contract, the state-dict key, ``reads_lowres`` and the config rule.

Reference: ``torch.nn.functional.cross_entropy`` itself, in f64 on the CPU.  ``cross_entropy_ref`` restates the formula of the
class docstring in f64 without calling it, and is pinned here against ``F.cross_entropy(x, y, weight=w, ignore_index=ii,
reduction=r, label_smoothing=e)``: both are f64 evaluations of the same few hundred terms, so they agree to a few ulp of f64 --
the bounds are 1e-12 relative for the loss and 1e-13 absolute for the gradient (entries of order 1 or below).  The restatement
exists because it also encodes the two deliberate deviations from torch (an out-of-range target counts as ignored; a zero divisor
gives loss 0 and gradient 0, not NaN), where torch cannot be the reference."""

import itertools

import pytest
import torch
import torch.nn.functional as F

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402


def cross_entropy_ref(logits, target, weight=None, ignore_index=-100, reduction="mean", label_smoothing=0.0):
    """L_i = (1-e) w_{y_i} (lse_i - x_{i,y_i}) + (e/K) sum_k w_k (lse_i - x_ik) over the valid pixels, divided by
    D = sum w_{y_i} for "mean" (0 where D == 0), in the dtype of ``logits``; an out-of-range target counts as ignored."""
    e, k = float(label_smoothing), logits.shape[1]
    w = torch.ones(k, dtype=logits.dtype) if weight is None else weight.to(logits.dtype)
    valid = (target >= 0) & (target < k)
    if ignore_index is not None:
        valid &= target != ignore_index
    y = torch.where(valid, target, torch.zeros_like(target))
    lse = torch.logsumexp(logits, dim=1)
    wy = w[y]
    hit = wy * (lse - logits.gather(1, y[:, None]).squeeze(1))
    smooth = ((lse[:, None] - logits) * w.view(1, k, *([1] * (logits.dim() - 2)))).sum(dim=1)
    per = (1.0 - e) * hit + (e / k) * smooth
    zero = torch.zeros_like(per)
    total = torch.where(valid, per, zero).sum()
    if reduction == "sum":
        return total
    d = torch.where(valid, wy, zero).sum()
    return total / d if d.item() > 0 else total * 0.0


def class_weights(k):
    """K class weights, all different, the third one zero, f32."""
    w = 0.5 + 0.25 * torch.arange(k, dtype=torch.float32)
    w[2 % k] = 0.0
    return w


# the option grid (shared with tests/test_hip_cross_entropy.py): weights, smoothing, ignore_index, reduction
GRID = [dict(weighted=wt, label_smoothing=e, ignore_index=ig, reduction=r)
        for wt, e, ig, r in itertools.product((False, True), (0.0, 0.1), (None, -100, 255), ("mean", "sum"))]


def grid_id(o):
    return f"{'w' if o['weighted'] else 'now'}-e{o['label_smoothing']}-ig{o['ignore_index']}-{o['reduction']}"


def ref_kwargs(o, k):
    """The keyword arguments of cross_entropy_ref for a GRID entry on k classes."""
    return dict(weight=class_weights(k) if o["weighted"] else None, ignore_index=o["ignore_index"], reduction=o["reduction"],
                label_smoothing=o["label_smoothing"])


def torch_kwargs(o, k):
    """The arguments of F.cross_entropy for a GRID entry: its ``ignore_index`` is an int, never None -- "no ignored pixel" is a
    value no target holds -- and its weight has the dtype of the logits (f64)."""
    kw = ref_kwargs(o, k)
    kw["ignore_index"] = -(2**40) if kw["ignore_index"] is None else kw["ignore_index"]
    kw["weight"] = None if kw["weight"] is None else kw["weight"].double()
    return kw


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("o", GRID, ids=grid_id)
def test_reference_formula_is_torch_cross_entropy(o):
    g = torch.Generator().manual_seed(3)
    k = 5
    x = (torch.randn(2, k, 7, 9, generator=g) * 3).double()
    y = torch.randint(0, k, (2, 7, 9), generator=g)
    if o["ignore_index"] is not None:
        y[torch.rand(y.shape, generator=g) < 0.2] = o["ignore_index"]
        assert 5 < (y == o["ignore_index"]).sum().item() < y.numel() // 2
    assert (y == 2).any(), "the zero-weight class is present"
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    mine = cross_entropy_ref(a, y, **ref_kwargs(o, k))
    kw = torch_kwargs(o, k)
    want = F.cross_entropy(b, y, **kw)
    assert torch.isfinite(want).item() and want.item() > 0
    assert abs(mine.item() - want.item()) <= 1e-12 * abs(want.item()), (mine.item(), want.item())
    mine.backward()
    want.backward()
    assert (a.grad - b.grad).abs().max().item() <= 1e-13
    # the gradient expression the kernels evaluate
    w = torch.ones(k, dtype=torch.float64) if kw["weight"] is None else kw["weight"].double()
    e = kw["label_smoothing"]
    valid = (y != kw["ignore_index"])
    ys = torch.where(valid, y, torch.zeros_like(y))
    wy = (w[ys] * valid)[:, None]
    onehot = F.one_hot(ys, k).permute(0, 3, 1, 2).double()
    closed = x.softmax(1) * ((1 - e) * wy + e / k * w.sum()) - (1 - e) * wy * onehot - e / k * w.view(1, k, 1, 1)
    closed = closed * valid[:, None] / (wy.sum() if kw["reduction"] == "mean" else 1.0)
    assert (a.grad - closed).abs().max().item() <= 1e-13
    if o["ignore_index"] is not None:
        assert (a.grad.permute(0, 2, 3, 1)[y == o["ignore_index"]] == 0).all()


def test_a_zero_weight_class_still_carries_the_smoothing_term():
    x = torch.tensor([[[[0.3]], [[-1.2]], [[2.0]]]], dtype=torch.float64)      # one pixel, three classes
    y = torch.tensor([[[1]]])
    w = torch.tensor([1.0, 0.0, 2.0])
    assert cross_entropy_ref(x, y, w, reduction="sum").item() == 0.0
    lse = torch.logsumexp(x[0, :, 0, 0], 0)
    want = (0.1 / 3) * (1.0 * (lse - 0.3) + 2.0 * (lse - 2.0))
    assert abs(cross_entropy_ref(x, y, w, reduction="sum", label_smoothing=0.1).item() - want.item()) <= 1e-15
    assert abs(F.cross_entropy(x, y, w.double(), reduction="sum", label_smoothing=0.1).item() - want.item()) <= 1e-15


def test_reference_encodes_the_two_deviations():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 4, 6, 6, generator=g).double()
    y = torch.randint(0, 4, (1, 6, 6), generator=g)
    w = class_weights(4)
    # 1. a target outside 0..K-1 that is not ignore_index counts as ignored
    bad, ign = y.clone(), y.clone()
    bad[0, :2] = 7
    bad[0, 2] = -3
    ign[0, :3] = -100
    for red in ("mean", "sum"):
        assert cross_entropy_ref(x, bad, w, -100, red, 0.1).item() == cross_entropy_ref(x, ign, w, -100, red, 0.1).item()
        assert abs(cross_entropy_ref(x, bad, w, -100, red, 0.1).item()
                   - F.cross_entropy(x, ign, w.double(), ignore_index=-100, reduction=red, label_smoothing=0.1).item()) <= 1e-12
    # 2. D == 0 with "mean": 0, not torch's NaN -- every pixel ignored, or every valid pixel of the zero-weight class
    for target in (torch.full_like(y, -100), torch.full_like(y, 2)):
        a = x.clone().requires_grad_(True)
        loss = cross_entropy_ref(a, target, w, -100, "mean", 0.1)
        loss.backward()
        assert loss.item() == 0.0 and (a.grad == 0).all()
        assert torch.isnan(F.cross_entropy(x, target, w.double(), ignore_index=-100, label_smoothing=0.1)).item()


# ------------------------------------------------------------------------------------------------ the class
def test_constructor_has_torch_signature_and_defaults():
    import inspect
    mine = inspect.signature(gnn.CrossEntropyLoss.__init__).parameters
    theirs = inspect.signature(torch.nn.CrossEntropyLoss.__init__).parameters
    assert list(mine) == list(theirs)
    for name in theirs:
        assert mine[name].default == theirs[name].default, name
    crit = gnn.CrossEntropyLoss()
    assert (crit.weight, crit.ignore_index, crit.reduction, crit.label_smoothing) == (None, -100, "mean", 0.0)
    assert crit._options(5) == ops.CrossEntropyOptions(0.0, -100, True, None) and crit._options(5).c_args() == (None, 0.0, 1, -100, 1)
    w = class_weights(5)
    crit = gnn.CrossEntropyLoss(w.double(), None, 255, None, "sum", 0.1)
    o = crit._options(5)
    assert crit.weight.dtype == torch.float32 and torch.equal(o.weight, w) and (o.label_smoothing, o.ignore_index, o.mean) == (0.1, 255, False)
    assert torch.equal(gnn.CrossEntropyLoss(weight=[1.0, 2.0]).weight, torch.tensor([1.0, 2.0]))
    assert ops.CrossEntropyOptions(ignore_index=None).c_args()[2:4] == (0, 0)


def test_constructor_rejects_what_the_issue_lists():
    with pytest.raises(NotImplementedError, match="implements"):
        gnn.CrossEntropyLoss(reduction="none")
    for kw in (dict(size_average=True), dict(size_average=False), dict(reduce=True), dict(reduce=False)):
        with pytest.raises(NotImplementedError, match="implements"):
            gnn.CrossEntropyLoss(**kw)
    for bad in ("median", "batchwise_mean", None):
        with pytest.raises(ValueError, match="reduction"):
            gnn.CrossEntropyLoss(reduction=bad)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="label_smoothing"):
            gnn.CrossEntropyLoss(label_smoothing=bad)
    for bad in (torch.ones(2, 3), torch.ones(()), torch.ones(3, 1, 1), torch.ones(0)):
        with pytest.raises(ValueError, match="1-D"):
            gnn.CrossEntropyLoss(weight=bad)
    for bad in ([1.0, -0.5], [1.0, float("nan")], [float("inf"), 1.0]):
        with pytest.raises(ValueError, match="finite and >= 0"):
            gnn.CrossEntropyLoss(weight=torch.tensor(bad))
    for bad in (2.5, True, 2**63):
        with pytest.raises(ValueError, match="ignore_index"):
            gnn.CrossEntropyLoss(ignore_index=bad)


def test_call_rejects_probability_targets_and_a_weight_of_the_wrong_length():
    x, y = torch.zeros(1, 5, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="class-index"):
        gnn.CrossEntropyLoss()(x, torch.zeros(1, 5, 4, 4))
    with pytest.raises(NotImplementedError, match="class-index"):
        gnn.CrossEntropyLoss()(gnn.LowresLogits(torch.zeros(1, 2, 2, 5), (4, 4)), torch.zeros(1, 4, 4))
    with pytest.raises(ValueError, match="for 5 classes"):
        gnn.CrossEntropyLoss(weight=torch.ones(4))(x, y)
    with pytest.raises(ValueError, match="for 5 classes"):
        gnn.CrossEntropyLoss(weight=torch.ones(6))(gnn.LowresLogits(torch.zeros(1, 2, 2, 5), (4, 4)), y)
    with pytest.raises(ValueError, match=r"\[B, K, H, W\]"):
        gnn.CrossEntropyLoss()(torch.zeros(4, 5), torch.zeros(4, dtype=torch.int64))


def test_state_dict_key_is_torchs():
    w = class_weights(5)
    crit = gnn.CrossEntropyLoss(weight=w)
    sd = crit.state_dict()
    assert list(sd) == ["weight"] and torch.equal(sd["weight"], w)
    assert list(sd) == list(torch.nn.CrossEntropyLoss(weight=w).state_dict())
    assert list(gnn.CrossEntropyLoss().state_dict()) == [] and gnn.CrossEntropyLoss().weight is None
    other = gnn.CrossEntropyLoss(weight=torch.zeros(5))
    other.load_state_dict(torch.nn.CrossEntropyLoss(weight=w).state_dict())
    assert torch.equal(other.weight, w) and torch.equal(other._options(5).weight, w)
    assert crit.double().weight.dtype == torch.float64 and crit._options(5).weight.dtype == torch.float32, "held as f32 for the kernels"


def test_reads_lowres_is_true_for_it_and_unchanged_for_the_other_losses():
    for n in (None, 1, 5):
        assert gnn.reads_lowres(gnn.CrossEntropyLoss(), n)
        assert gnn.reads_lowres(gnn.CrossEntropyLoss(weight=class_weights(5), label_smoothing=0.1, reduction="sum"), n)
        assert not gnn.reads_lowres(torch.nn.CrossEntropyLoss(), n) and not gnn.reads_lowres(torch.nn.BCEWithLogitsLoss(), n)
        assert gnn.reads_lowres(gnn.SoftCrossEntropyLoss(smooth_factor=0.1), n)
        assert not gnn.reads_lowres(gnn.LovaszLoss("multiclass"), n)
    for cls in (gnn.DiceLoss, gnn.JaccardLoss, gnn.TverskyLoss, gnn.FocalLoss):
        assert gnn.reads_lowres(cls("multiclass")) and not gnn.reads_lowres(cls("binary")) and gnn.reads_lowres(cls("binary"), 1)
    assert gnn.reads_lowres(gnn.SoftBCEWithLogitsLoss(), 1) and not gnn.reads_lowres(gnn.SoftBCEWithLogitsLoss(), 5)


def test_config_leaves_torchs_class_unaliased_and_names_the_hip_loss():
    from geo_deep_learning import train as gdl_train
    assert not any(k.startswith("torch.") for k in gdl_train.CLASS_ALIASES)
    crit = gdl_train.instantiate({"class_path": "torch.nn.CrossEntropyLoss", "init_args": {"ignore_index": 255}})
    assert type(crit) is torch.nn.CrossEntropyLoss and crit.ignore_index == 255
    crit = gdl_train.instantiate({"class_path": "gdlhip.nn.CrossEntropyLoss",
                                  "init_args": {"weight": [0.2, 1.0, 1.0, 2.0, 2.0], "ignore_index": 255, "label_smoothing": 0.1}})
    assert type(crit) is gnn.CrossEntropyLoss and (crit.ignore_index, crit.label_smoothing, crit.reduction) == (255, 0.1, "mean")
    assert torch.equal(crit.weight, torch.tensor([0.2, 1.0, 1.0, 2.0, 2.0]))
    assert "gdlhip.nn.CrossEntropyLoss" in gdl_train.__doc__


def test_ops_and_class_refuse_cpu_tensors():
    x, y = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    low, up, norm = torch.zeros(1, 2, 2, 3), torch.ones(()), torch.ones(1)
    for call in (lambda: ops.cross_entropy_fwd(x, y), lambda: ops.cross_entropy_bwd(x, y, norm, up),
                 lambda: ops.cross_entropy_lowres_fwd(low, y, (4, 4)), lambda: ops.cross_entropy_lowres_bwd(low, y, (4, 4), norm, up),
                 lambda: gnn.CrossEntropyLoss()(x, y), lambda: gnn.CrossEntropyLoss(weight=torch.ones(3))(x, y)):
        with pytest.raises(ValueError):
            call()
    assert ops.cross_entropy_lowres_ok(torch.zeros(1, 2, 2, 16), (128, 128)) and not ops.cross_entropy_lowres_ok(torch.zeros(1, 2, 2, 17), (4, 4))
    assert not ops.cross_entropy_lowres_ok(torch.zeros(1, 8, 8, 5), (4, 4)) and not ops.cross_entropy_lowres_ok(torch.zeros(1, 2, 2, 5), (130, 4))
