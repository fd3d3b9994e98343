"""The autograd layer of the losses in gdlhip.nn without a GPU: with every ``ops.*_fwd`` / ``*_bwd`` of the loss ops replaced by a
recorder that returns CPU tensors of the right shapes, every loss module is driven over every kind of input it accepts and
``.backward()`` is called on the result.  Pinned: which forward and backward op ran, what each received (f32 contiguous input, the
squeezed / converted target, ``size``, ``eps``, ``options``, the forward's state tensors, an f32 upstream, ``grad_scale`` 1.0),
that the input got a gradient of its own shape, and in which cases ``LowresLogits.materialise()`` ran.  Autograd itself rejects a
wrong number of returned gradients, so the ``None`` counts of every route are pinned too.  Smallest shapes: B=2, K=3, 4x4 -> 8x8."""

import inspect

import pytest
import torch
import torch.nn.functional as F

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402

SIZE = (8, 8)
# op stem -> the names of the state tensors its forward returns behind the loss (and its backward takes)
STEMS = {"dice_loss": ("sums",), "dice_loss_lowres": ("sums",), "dice_binary_loss": ("sums",), "dice_binary_lowres": ("sums",),
         "soft_ce": (), "soft_ce_lowres": ("state",), "cross_entropy": ("norm",), "cross_entropy_lowres": ("norm",),
         "focal": ("norm",), "focal_binary": ("norm",), "focal_lowres": ("norm",), "focal_binary_lowres": ("norm",),
         "soft_bce": (), "soft_bce_lowres": (), "lovasz": ("coef", "norm"), "lovasz_binary": ("coef", "norm")}


class Trace:
    def __init__(self):
        self.calls, self.returned, self.materialised = [], {}, 0


@pytest.fixture
def trace(monkeypatch):
    t = Trace()

    def record(name, real):
        sig = inspect.signature(real)

        def fake(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            args = dict(bound.arguments)
            t.calls.append((name, args))
            first = next(iter(args.values()))
            if name.endswith("_bwd"):
                return torch.ones_like(first)
            stem = name[:-4]
            states = [torch.full((3 + i,), float(i)) for i in range(len(STEMS[stem]))]
            if stem == "soft_ce_lowres" and not args["fused"]:
                states = [None]
            t.returned[stem] = states
            return (torch.zeros(()), *states) if (states or stem == "soft_ce_lowres") else torch.zeros(())

        monkeypatch.setattr(ops, name, fake)

    for stem in STEMS:
        for way in ("_fwd", "_bwd"):
            record(stem + way, getattr(ops, stem + way))

    def materialise(self):
        t.materialised += 1
        return F.interpolate(self.low.float().permute(0, 3, 1, 2), size=self.size, mode="bilinear", align_corners=False)

    monkeypatch.setattr(gnn.LowresLogits, "materialise", materialise)
    return t


def _pred(kind: str):
    """(the leaf that must receive the gradient, what the loss is called with)"""
    kind, _, how = kind.partition(":")
    dtype = torch.bfloat16 if how == "bf16" else torch.float32
    if kind == "flat":
        leaf = torch.randn(2, 64, requires_grad=True)
        return leaf, leaf
    k = int(kind[-1])
    if kind.startswith("low"):
        leaf = torch.randn(2, 4, 4, k, dtype=dtype, requires_grad=how != "nograd")
        return leaf, gnn.LowresLogits(leaf, SIZE)
    if how == "strided":
        leaf = torch.randn(2, 8, 8, k, requires_grad=True)
        return leaf, leaf.permute(0, 3, 1, 2)
    leaf = torch.randn(2, k, 8, 8, dtype=dtype, requires_grad=True)
    return leaf, leaf


TARGETS = {"y": lambda: torch.zeros(2, 8, 8, dtype=torch.int64), "y1": lambda: torch.zeros(2, 1, 8, 8, dtype=torch.int64),
           "y16": lambda: torch.zeros(2, 16, 16, dtype=torch.int64), "yi32": lambda: torch.zeros(2, 8, 8, dtype=torch.int32),
           "yf": lambda: torch.zeros(2, 8, 8), "yf64": lambda: torch.zeros(2, 1, 8, 8, dtype=torch.float64),
           "yk": lambda: torch.zeros(2, 3, 8, 8), "yflat": lambda: torch.zeros(2, 64, dtype=torch.int64)}

W5 = [0.25, 1.0, 2.0]
CRITS = {
    "dice": lambda: gnn.DiceLoss(smooth=1.0, eps=3e-5), "dice-plain": lambda: gnn.DiceLoss(), "jaccard": lambda: gnn.JaccardLoss(eps=3e-5),
    "tversky": lambda: gnn.TverskyLoss(ignore_index=255, alpha=0.3, beta=0.7), "dice-bin": lambda: gnn.DiceLoss(mode="binary", eps=3e-5),
    "tversky-bin": lambda: gnn.TverskyLoss(mode="binary"), "soft_ce": lambda: gnn.SoftCrossEntropyLoss(smooth_factor=0.1),
    "xent": lambda: gnn.CrossEntropyLoss(weight=torch.tensor(W5), ignore_index=255, label_smoothing=0.1),
    "xent-plain": lambda: gnn.CrossEntropyLoss(reduction="sum"),
    "focal": lambda: gnn.FocalLoss("multiclass", alpha=0.25), "focal-bin": lambda: gnn.FocalLoss("binary", alpha=0.25),
    "soft_bce": lambda: gnn.SoftBCEWithLogitsLoss(smooth_factor=0.1, ignore_index=255, pos_weight=torch.tensor([1.5])),
    "soft_bce-plain": lambda: gnn.SoftBCEWithLogitsLoss(),
    "lovasz": lambda: gnn.LovaszLoss("multiclass", ignore_index=255), "lovasz-bin": lambda: gnn.LovaszLoss("binary", per_image=True),
}

MAT = dict(mat=1)      # the low-resolution logits were materialised
OFF = dict(mat=1, off=True)      # ... because FUSE_LOWRES_DICE is off


def _multiclass(crit: str, full: str, low: str, one_class_low: bool = True):
    """The input kinds of a K-class loss: ``full`` is the op stem on [B, K, H, W] logits, ``low`` on LowresLogits."""
    rows = [(crit, "nchw3", "y", full, {}), (crit, "nchw3", "y1", full, {}), (crit, "nchw3:bf16", "y", full, {}),
            (crit, "nchw3:strided", "y", full, {}), (crit, "low3", "y", low, {}), (crit, "low3", "y1", low, {}),
            (crit, "low3:bf16", "y", full, MAT), (crit, "low3", "y16", full, dict(mat=1, tshape=(2, 16, 16))), (crit, "low3", "y", full, OFF)]
    if one_class_low:
        rows.append((crit, "low1", "y", low, {}))
    return rows


def _binary(crit: str, full: str, low: str):
    """The input kinds of a one-class (binary) loss; the full-resolution ops take the target as it comes (any shape of the logits'
    numel), the low-resolution ones [B, H, W]."""
    return [(crit, "nchw1", "y", full, {}), (crit, "nchw1", "y1", full, dict(tshape=(2, 1, 8, 8))), (crit, "nchw1:bf16", "y", full, {}),
            (crit, "nchw1:strided", "y1", full, dict(tshape=(2, 1, 8, 8))), (crit, "low1", "y", low, {}), (crit, "low1", "y1", low, {}),
            (crit, "low1:bf16", "y", full, MAT), (crit, "low1", "y", full, OFF),
            (crit, "low3", "y", full, dict(mat=1, raises="do not match"))]


CASES = (
    _multiclass("dice", "dice_loss", "dice_loss_lowres") + _multiclass("dice-plain", "dice_loss", "dice_loss_lowres")[:5]
    + _multiclass("jaccard", "dice_loss", "dice_loss_lowres")[:5] + _multiclass("tversky", "dice_loss", "dice_loss_lowres")[:5]
    + _binary("dice-bin", "dice_binary_loss", "dice_binary_lowres") + _binary("tversky-bin", "dice_binary_loss", "dice_binary_lowres")[:5]
    + _multiclass("soft_ce", "soft_ce", "soft_ce_lowres") + _multiclass("xent", "cross_entropy", "cross_entropy_lowres", False)
    + _multiclass("xent-plain", "cross_entropy", "cross_entropy_lowres")[:5]
    + _multiclass("focal", "focal", "focal_lowres") + _binary("focal-bin", "focal_binary", "focal_binary_lowres")
    + _binary("soft_bce", "soft_bce", "soft_bce_lowres")
    + [("soft_bce", "nchw1", "yf", "soft_bce", dict(tdtype=torch.float32)), ("soft_bce", "nchw1", "yi32", "soft_bce", {}),
       ("soft_bce", "nchw1", "yf64", "soft_bce", dict(tdtype=torch.float32, tshape=(2, 1, 8, 8))),
       ("soft_bce-plain", "nchw3", "yk", "soft_bce", dict(tdtype=torch.float32, tshape=(2, 3, 8, 8))),
       ("soft_bce-plain", "flat", "yflat", "soft_bce", dict(pshape=(2, 1, 1, 64), tshape=(2, 64))),
       ("soft_bce", "low1", "yf", "soft_bce_lowres", dict(tdtype=torch.float32)),
       ("soft_bce", "low1", "yi32", "soft_bce_lowres", {})]
    + [(c, p, t, "lovasz", dict(mat=int(p.startswith("low")))) for c, p, t, _, _ in _multiclass("lovasz", "", "")[:7]]
    + [("lovasz-bin", "nchw1", "y", "lovasz_binary", {}), ("lovasz-bin", "nchw1", "y1", "lovasz_binary", dict(tshape=(2, 1, 8, 8))),
       ("lovasz-bin", "nchw1:bf16", "y", "lovasz_binary", {}), ("lovasz-bin", "low1", "y", "lovasz_binary", MAT),
       ("lovasz-bin", "low3", "y", "lovasz_binary", dict(mat=1, raises="do not match"))]
)


def _same(a, b) -> bool:
    return a is b or (a is not None and b is not None and a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype)


def _check_options(crit, got):
    if isinstance(crit, gnn.CrossEntropyLoss):
        assert isinstance(got, ops.CrossEntropyOptions)
        assert got[:3] == (crit.label_smoothing, crit.ignore_index, crit.reduction == "mean")
        assert (got.weight is None) if crit.weight is None else torch.equal(got.weight, crit.weight)
    elif isinstance(crit, gnn.SoftBCEWithLogitsLoss):
        assert isinstance(got, ops.SoftBCEOptions)
        assert got[:3] == (crit.smooth_factor, crit.ignore_index, crit.reduction == "mean")
        for g, w in ((got.weight, crit.weight), (got.pos_weight, crit.pos_weight)):
            assert (g is None) if w is None else torch.equal(g, w)
    else:
        assert got is crit.options


@pytest.mark.parametrize("crit,pred,target,stem,extra", CASES,
                         ids=[f"{c}-{p}-{t}{'-off' if e.get('off') else ''}" for c, p, t, _, e in CASES])
def test_route_arguments_and_gradient(trace, monkeypatch, crit, pred, target, stem, extra):
    monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", not extra.get("off", False))
    monkeypatch.setattr(gnn, "SOFT_CE_LOWRES_FUSED", True)
    crit = CRITS[crit]()
    leaf, y_pred = _pred(pred)
    y_true = TARGETS[target]()
    if "raises" in extra:
        with pytest.raises(ValueError, match=extra["raises"]):
            crit(y_pred, y_true)
        assert trace.materialised == extra["mat"] and trace.calls == []
        return
    loss = crit(y_pred, y_true)
    assert trace.materialised == extra.get("mat", 0)
    assert [c[0] for c in trace.calls] == [stem + "_fwd"]
    loss.backward()
    assert [c[0] for c in trace.calls] == [stem + "_fwd", stem + "_bwd"]
    assert trace.materialised == extra.get("mat", 0)
    fwd, bwd = trace.calls[0][1], trace.calls[1][1]
    lowres = stem.endswith("_lowres")
    k = int(pred.partition(":")[0][-1]) if pred != "flat" else 1

    x, t = list(fwd.values())[:2]
    assert x.dtype == torch.float32 and x.is_contiguous()
    assert tuple(x.shape) == extra.get("pshape", (2, 4, 4, k) if lowres else (2, k, 8, 8))
    assert t.dtype == extra.get("tdtype", torch.int64) and t.is_contiguous() and tuple(t.shape) == extra.get("tshape", (2, 8, 8))
    assert ("size" in fwd) == lowres and ("size" in bwd) == lowres
    if lowres:
        assert fwd["size"] == SIZE and bwd["size"] == SIZE and all(type(v) is int for v in fwd["size"])
    assert ("eps" in fwd) == stem.startswith("dice") and ("eps" in bwd) == stem.startswith("dice")
    if "eps" in fwd:
        assert fwd["eps"] == crit.eps and bwd["eps"] == crit.eps
    _check_options(crit, fwd["options"])
    assert bwd["options"] is fwd["options"]
    if stem == "soft_ce_lowres":
        assert fwd["fused"] is True and trace.returned[stem][0] is not None

    bx, bt = list(bwd.values())[:2]
    assert _same(bx, x) and _same(bt, t)
    assert len(trace.returned[stem]) == len(STEMS[stem])
    for name, want in zip(STEMS[stem], trace.returned[stem]):
        assert _same(bwd[name], want), name
    up = bwd["upstream"]
    assert up.dtype == torch.float32 and up.is_contiguous() and up.shape == () and up.item() == 1.0
    assert type(bwd["grad_scale"]) is float and bwd["grad_scale"] == 1.0
    for key, default in (("out", None), ("accumulate", False), ("form", "auto")):      # the autograd layer sets none of them
        assert key not in bwd or bwd[key] is default or bwd[key] == default
    assert leaf.grad is not None and leaf.grad.shape == leaf.shape and leaf.grad.dtype == leaf.dtype
    assert leaf.grad.abs().sum().item() > 0


@pytest.mark.parametrize("switch,needs_grad", [(True, True), (True, False), (False, True)])
def test_soft_ce_lowres_asks_for_the_fused_forward_only_when_a_backward_will_follow(trace, monkeypatch, switch, needs_grad):
    """``fused`` is SOFT_CE_LOWRES_FUSED and needs_input_grad[0]; without it the forward returns no state and the backward gets
    ``state=None``."""
    monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", True)
    monkeypatch.setattr(gnn, "SOFT_CE_LOWRES_FUSED", switch)
    crit = gnn.SoftCrossEntropyLoss(smooth_factor=0.1)
    leaf, y_pred = _pred("low3" if needs_grad else "low3:nograd")
    loss = crit(y_pred, TARGETS["y"]())
    fwd = trace.calls[0][1]
    assert trace.calls[0][0] == "soft_ce_lowres_fwd" and fwd["fused"] is (switch and needs_grad)
    if not needs_grad:
        assert not loss.requires_grad and len(trace.calls) == 1
        return
    loss.backward()
    name, bwd = trace.calls[1]
    assert name == "soft_ce_lowres_bwd" and (bwd["state"] is not None) == switch
    assert switch is False or _same(bwd["state"], trace.returned["soft_ce_lowres"][0])
    assert leaf.grad.shape == leaf.shape


def test_cross_entropy_refuses_floating_targets_before_anything_else(trace):
    with pytest.raises(NotImplementedError, match="class-index targets"):
        gnn.CrossEntropyLoss()(_pred("low3")[1], TARGETS["yf"]())
    assert trace.calls == [] and trace.materialised == 0


def test_dice_family_checks_its_classes_against_the_logits(trace, monkeypatch):
    monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", True)
    crit = gnn.DiceLoss(classes=[0, 3])
    for pred in ("nchw3", "low3"):
        with pytest.raises(ValueError, match="out of range for 3 classes"):
            crit(_pred(pred)[1], TARGETS["y"]())
    assert trace.calls == [] and trace.materialised == 0


@pytest.mark.parametrize("crit,match", [("soft_ce", r"SoftCrossEntropyLoss: \[B, K, H, W\] logits expected"),
                                        ("xent", r"CrossEntropyLoss: \[B, K, H, W\] logits expected"),
                                        ("focal", r"FocalLoss\(multiclass\): \[B, K, H, W\] logits expected"),
                                        ("lovasz", r"LovaszLoss\(multiclass\): \[B, K, H, W\] logits expected")])
def test_the_multiclass_losses_name_themselves_when_the_logits_are_not_4d(trace, crit, match):
    with pytest.raises(ValueError, match=match):
        CRITS[crit]()(torch.zeros(2, 8, 8), TARGETS["y"]())
    assert trace.calls == []
