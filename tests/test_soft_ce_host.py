"""gdlhip.nn.SoftCrossEntropyLoss, the parts that need no GPU: constructor contract, the reference formula the GPU tests hold the
kernels against, the config alias, and the host logic by which SegmentationDOFA hands the loss low-resolution logits.

Reference: smp 0.5.0 losses/soft_ce.py + losses/_functional.py::label_smoothed_nll_loss restated in f64 (``soft_ce_ref``).  smp
itself is not available, so parity with it is unpinned; what is pinned is the identity
``soft_ce_ref(x, y) == F.cross_entropy(x, y, ignore_index=ii, label_smoothing=e, reduction="sum") [/ N]``, an implementation
that shares no code with the kernels or with the restatement."""

from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402


def soft_ce_ref(logits, target, smooth_factor=None, ignore_index=-100, reduction="mean"):
    """The formula of the class docstring in the dtype of ``logits``; an out-of-range target counts as ignored."""
    e = 0.0 if smooth_factor is None else float(smooth_factor)
    k = logits.shape[1]
    valid = (target >= 0) & (target < k)
    if ignore_index is not None:
        valid &= target != ignore_index
    y = torch.where(valid, target, torch.zeros_like(target))
    lse = torch.logsumexp(logits, dim=1)
    xy = logits.gather(1, y[:, None]).squeeze(1)
    per = lse - (1.0 - e) * xy - (e / k) * logits.sum(dim=1)
    total = torch.where(valid, per, torch.zeros_like(per)).sum()
    return total / target.numel() if reduction == "mean" else total


def test_constructor_accepts_smp_arguments_and_rejects_the_rest():
    crit = gnn.SoftCrossEntropyLoss()
    assert (crit.reduction, crit.smooth_factor, crit.ignore_index, crit.dim) == ("mean", None, -100, 1)
    assert crit.options == ops.SoftCEOptions(0.0, -100, True)
    crit = gnn.SoftCrossEntropyLoss(reduction="sum", smooth_factor=0.1, ignore_index=255)
    assert crit.options == ops.SoftCEOptions(0.1, 255, False) and crit.options.c_args() == (0.1, 1, 255, 0)
    assert gnn.SoftCrossEntropyLoss(ignore_index=None).options.c_args() == (0.0, 0, 0, 1)
    assert gnn.SoftCrossEntropyLoss(smooth_factor=0).options.smooth_factor == 0.0
    assert gnn.SoftCrossEntropyLoss(smooth_factor=1.0).options.smooth_factor == 1.0
    with pytest.raises(NotImplementedError):
        gnn.SoftCrossEntropyLoss(reduction="none")
    with pytest.raises(NotImplementedError):
        gnn.SoftCrossEntropyLoss(dim=-1)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gnn.SoftCrossEntropyLoss(smooth_factor=bad)
    for bad in (2.5, True, 2**63):
        with pytest.raises(ValueError):
            gnn.SoftCrossEntropyLoss(ignore_index=bad)
    with pytest.raises(ValueError):
        gnn.SoftCrossEntropyLoss(reduction="median")


def test_ops_refuse_cpu_tensors():
    x, y = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    low = torch.zeros(1, 2, 2, 3)
    up = torch.ones(())
    with pytest.raises(ValueError):
        ops.soft_ce_fwd(x, y)
    with pytest.raises(ValueError):
        ops.soft_ce_bwd(x, y, up)
    with pytest.raises(ValueError):
        ops.soft_ce_lowres_fwd(low, y, (4, 4))
    with pytest.raises(ValueError):
        ops.soft_ce_lowres_bwd(low, y, (4, 4), up)
    with pytest.raises(ValueError):
        gnn.SoftCrossEntropyLoss()(x, y)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("ignore", [None, -100, 255])
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_reference_formula_is_torch_cross_entropy_summed_over_n(eps, ignore, reduction):
    """soft_ce_ref == F.cross_entropy(label_smoothing=eps, reduction="sum") [/ N] in f64, loss and gradient, with and without
    ignored pixels.  N counts every pixel: with ignored pixels present the mean differs from torch's own "mean"."""
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(2, 5, 13, 11, generator=g) * 3).double()
    y = torch.randint(0, 5, (2, 13, 11), generator=g)
    if ignore is not None:
        y[torch.rand(y.shape, generator=g) < 0.2] = ignore
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    mine = soft_ce_ref(a, y, eps, ignore, reduction)
    want = F.cross_entropy(b, y, ignore_index=-(2**40) if ignore is None else ignore, label_smoothing=eps, reduction="sum")
    if reduction == "mean":
        want = want / y.numel()
    assert abs(mine.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
    mine.backward()
    want.backward()
    assert (a.grad - b.grad).abs().max().item() <= 1e-14
    k = x.shape[1]
    onehot = F.one_hot(y.clamp(0, k - 1), k).permute(0, 3, 1, 2).double()
    valid = ((y >= 0) & (y < k))[:, None].double()
    closed = valid * (x.softmax(1) - (1 - eps) * onehot - eps / k) / (y.numel() if reduction == "mean" else 1)
    assert (a.grad - closed).abs().max().item() <= 1e-14, "the gradient expression the kernels evaluate"
    if ignore is not None and reduction == "mean":
        torch_mean = F.cross_entropy(x, y, ignore_index=ignore, label_smoothing=eps)
        assert abs(torch_mean.item() - mine.item()) > 1e-3, "smp's mean divides by N, torch's by the valid count"


def test_reference_treats_an_out_of_range_target_as_ignored():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 4, 6, 6, generator=g).double()
    y = torch.randint(0, 4, (1, 6, 6), generator=g)
    bad = y.clone()
    bad[0, :2] = 7
    bad[0, 2] = -3
    ign = y.clone()
    ign[0, :3] = -100
    assert soft_ce_ref(x, bad, 0.1).item() == soft_ce_ref(x, ign, 0.1).item()


def test_config_alias_resolves_to_the_hip_loss():
    from geo_deep_learning import train as gdl_train
    crit = gdl_train.instantiate({"class_path": "segmentation_models_pytorch.losses.SoftCrossEntropyLoss",
                                  "init_args": {"smooth_factor": 0.1}})
    assert type(crit) is gnn.SoftCrossEntropyLoss and crit.options.smooth_factor == pytest.approx(0.1)


def test_reads_lowres_names_the_losses_that_take_low_resolution_logits():
    assert gnn.reads_lowres(gnn.SoftCrossEntropyLoss(smooth_factor=0.1))
    assert gnn.reads_lowres(gnn.DiceLoss(mode="multiclass"))
    assert not gnn.reads_lowres(gnn.DiceLoss(mode="binary"))
    assert not gnn.reads_lowres(torch.nn.CrossEntropyLoss())


def test_dofa_task_hands_the_loss_low_resolution_logits(monkeypatch):
    """SegmentationDOFA with SoftCrossEntropyLoss asks the model for ``lowres_logits=True`` in training and validation, and for
    the resized logits when GDL_LOWRES_DICE=0 (gnn.FUSE_LOWRES_DICE off) switches both losses off that path."""
    from tasks_with_models.segmentation_dofa import SegmentationDOFA
    calls = []

    class Model(torch.nn.Module):
        def forward(self, x, wv, lowres_logits=False):
            calls.append(bool(lowres_logits))
            out = torch.zeros(x.shape[0], 5, 8, 8, requires_grad=True)
            return SimpleNamespace(out=out, aux=out)

    class FakeCE(gnn.SoftCrossEntropyLoss):      # the class the predicate tests for; no kernel behind it here
        def forward(self, y_pred, y_true):
            return y_pred.sum() * 0.0

    def task_with(loss):
        t = SegmentationDOFA("dofa_base", pretrained=False, image_size=(8, 8), num_classes=5, max_samples=1, loss=loss)
        t.model = Model()
        return t

    batch = {"image": torch.zeros(2, 3, 8, 8), "mask": torch.zeros(2, 1, 8, 8, dtype=torch.int64),
             "wavelengths": torch.tensor([0.6, 0.5, 0.4])}
    monkeypatch.setattr(gnn, "predict_mask", lambda logits: logits.argmax(1))      # (the mask kernel needs a GPU)
    monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", True)
    t = task_with(FakeCE(smooth_factor=0.1))
    t.training_step(batch, 0)
    with torch.no_grad():
        t.validation_step(batch, 0)
    assert calls == [True, True]
    calls.clear()
    monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", False)
    t = task_with(FakeCE(smooth_factor=0.1))
    t.training_step(batch, 0)
    with torch.no_grad():
        t.validation_step(batch, 0)
    assert calls == [False, False]
