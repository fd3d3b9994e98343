"""gdlhip.nn.DiceLoss with smp's constructor options (ignore_index, smooth, log_loss, classes) evaluated inside the HIP
kernels: the full-resolution, low-resolution (LowresLogits) and binary families, forward and backward.

The reference of every number is ``dice_ref`` below: smp 0.5.0 losses/dice.py restated in f64 with plain torch CPU ops,
gradients from torch autograd; for the low-resolution family it is applied to ``F.interpolate(low, size, "bilinear")``.
``test_reference_formula_equals_the_oracle`` ties it to oracle.model.dice_loss_* (the formula the goldens were held against).

Tolerances are those of the Dice tests in test_hip_ops.py: loss within 1e-6 of the f64 reference (2e-6 from low-resolution
logits), gradients within 1e-4 of max|ref| (``close``).  With ``log_loss`` the loss bound is divided by the smallest
``score_k`` of a present, selected class, because -log divides the error of score_k by score_k.

The host tests (constructor, reference formula, struct layout) run without a GPU; the others are marked ``gpu``."""

import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"
UP = 0.4          # the upstream factor of the auxiliary head
LOSS_TOL, LOSS_TOL_LOWRES, GRAD_TOL = 1e-6, 2e-6, 1e-4


# ------------------------------------------------------------------------------------------------ reference
def dice_ref(logits, target, mode="multiclass", ignore_index=None, smooth=0.0, log_loss=False, classes=None, eps=1e-7):
    """smp 0.5.0 DiceLoss in the dtype of ``logits`` (f64 in these tests): (loss, score_k, Y_k)."""
    b = logits.shape[0]
    y = target.reshape(b, -1)
    if mode == "multiclass":
        k = logits.shape[1]
        p = logits.softmax(dim=1).reshape(b, k, -1)
        hot = torch.stack([(y == c) for c in range(k)], dim=1).to(p.dtype)
    else:
        p = F.logsigmoid(logits).exp().reshape(b, 1, -1)
        hot = y.reshape(b, 1, -1).to(p.dtype)
    valid = torch.ones_like(y, dtype=p.dtype) if ignore_index is None else (y != ignore_index).to(p.dtype)
    valid = valid[:, None, :]
    inter = (valid * p * hot).sum(dim=(0, 2))
    psum = (valid * p).sum(dim=(0, 2))
    ysum = (valid * hot).sum(dim=(0, 2))
    score = (2.0 * inter + smooth) / (psum + ysum + smooth).clamp_min(eps)
    loss = -torch.log(score.clamp_min(eps)) if log_loss else 1.0 - score
    loss = loss * (ysum > 0).to(p.dtype)
    if classes is not None:
        loss = loss[list(classes)]
    return loss.mean(), score.detach(), ysum.detach()


def loss_bound(base, kw, score, ysum):
    """The loss tolerance: ``base``, divided by the smallest score of a present, selected class with log_loss."""
    if not kw.get("log_loss"):
        return base
    sel = list(kw["classes"]) if kw.get("classes") is not None else list(range(score.numel()))
    present = [score[c].item() for c in sel if ysum[c] > 0]
    return base / min(present) if present else base


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)))


def make_target(shape, k, ignore=None, frac=0.2, seed=1, absent=True):
    """Class indices 0..k-2 (class k-1 absent) with about ``frac`` of the pixels set to ``ignore``."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, max(k - 1, 1) if absent else k, shape, generator=g)
    if ignore is not None:
        t[torch.rand(shape, generator=g) < frac] = ignore
    return t


def grad_close(got, ref, what):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    s = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    print(f"{what}: grad max err {err:.3e} vs scale {s:.3e}")
    assert err <= GRAD_TOL * s, f"{what}: grad max err {err:.3e} vs scale {s:.3e}"


def check_full(logits, target, mode="multiclass", **kw):
    """DiceLoss(mode, **kw) on full-resolution logits, forward and backward with the upstream factor, against dice_ref."""
    x = logits.double().clone().requires_grad_(True)
    ref, score, ysum = dice_ref(x, target, mode, **kw)
    (UP * ref).backward()
    ld = logits.to(DEV).requires_grad_(True)
    loss = gnn.DiceLoss(mode=mode, **kw)(ld, target.to(DEV))
    (UP * loss).backward()
    bound = loss_bound(LOSS_TOL, kw, score, ysum)
    err = abs(loss.item() - ref.item())
    print(f"{mode} {kw}: loss {loss.item():.8f} ref {ref.item():.8f} err {err:.3e} bound {bound:.3e}")
    assert torch.isfinite(loss).item() and torch.isfinite(ld.grad).all().item()
    assert err <= bound
    grad_close(ld.grad, x.grad, f"{mode} {kw}")
    return loss, ld.grad


def check_lowres(shape, tiled=True, **kw):
    """DiceLoss(**kw) on LowresLogits: against dice_ref on the interpolated logits, and against the materialised path."""
    B, K, hi, wi, ho, wo = shape
    low = rnd(B, hi, wi, K, seed=3) * 2.0
    ign = kw.get("ignore_index")
    tgt = make_target((B, ho, wo), K, ign, seed=4)
    lr = low.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref, score, ysum = dice_ref(F.interpolate(lr, size=(ho, wo), mode="bilinear", align_corners=False), tgt, **kw)
    (UP * ref).backward()
    lowd, tgtd = low.to(DEV), tgt.to(DEV)
    crit = gnn.DiceLoss(mode="multiclass", **kw)
    a = lowd.clone().requires_grad_(True)
    b_ = lowd.clone().requires_grad_(True)
    lib = gdlhip._lib.load()
    lib.gdl_debug_set_dice_lowres_tiled(1 if tiled else 0)
    try:
        takes_tiles = lib.gdl_dice_loss_lowres_bwd_workspace(B, K, hi, wi, ho, wo) > 0
        la = crit(gnn.LowresLogits(a, (ho, wo)), tgtd)
        (UP * la).backward()
    finally:
        lib.gdl_debug_set_dice_lowres_tiled(1)
    lb = crit(gnn.LowresLogits(b_, (ho, wo)).materialise(), tgtd)
    (UP * lb).backward()
    bound = loss_bound(LOSS_TOL_LOWRES, kw, score, ysum)
    err = abs(la.item() - ref.item())
    print(f"lowres {shape} tiled={takes_tiles} {kw}: loss {la.item():.8f} ref {ref.item():.8f} err {err:.3e} bound {bound:.3e}; "
          f"vs materialised {abs(la.item() - lb.item()):.3e}")
    assert torch.isfinite(la).item() and torch.isfinite(a.grad).all().item()
    assert err <= bound
    assert abs(la.item() - lb.item()) <= loss_bound(LOSS_TOL, kw, score, ysum)
    grad_close(a.grad.permute(0, 3, 1, 2), lr.grad, f"lowres {shape} {kw} vs torch")
    grad_close(a.grad, b_.grad, f"lowres {shape} {kw} vs the materialised path")
    return la, a.grad, takes_tiles


# ------------------------------------------------------------------------------------------------ host tests (no GPU)
def test_constructor_accepts_the_options_and_rejects_what_is_not_implemented():
    crit = gnn.DiceLoss(mode="multiclass", classes=[1, 3], log_loss=True, smooth=1.0, ignore_index=255)
    assert crit.classes == (1, 3) and crit.log_loss and crit.smooth == 1.0 and crit.ignore_index == 255
    assert crit.options == ops.DiceOptions(255, 1.0, True, (1, 3))
    assert gnn.DiceLoss(ignore_index=-100).options.ignore_index == -100
    assert gnn.DiceLoss(mode="binary", classes=[0], smooth=1.0).options.classes == (0,)
    # smp's defaults, spelled out or not, take the plain kernels
    assert gnn.DiceLoss().options is None
    assert gnn.DiceLoss(ignore_index=None, smooth=0.0, log_loss=False, classes=None).options is None
    with pytest.raises(NotImplementedError):
        gnn.DiceLoss(from_logits=False)
    with pytest.raises(NotImplementedError):
        gnn.DiceLoss(mode="multilabel")
    with pytest.raises(ValueError):
        gnn.DiceLoss(classes=[1, 1])
    with pytest.raises(ValueError):
        gnn.DiceLoss(classes=[-1, 2])
    with pytest.raises(ValueError):
        gnn.DiceLoss(mode="binary", classes=[1])
    with pytest.raises(ValueError):
        gnn.DiceLoss(ignore_index=2.5)
    # the range of `classes` is checked when K is known (before any kernel is launched)
    with pytest.raises(ValueError, match="out of range"):
        gnn.DiceLoss(classes=[1, 7])(torch.zeros(1, 5, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))


def test_reference_formula_equals_the_oracle():
    """dice_ref with default options (and with smooth alone) is oracle.model.dice_loss_multiclass / dice_loss_binary."""
    from oracle.model import dice_loss_binary, dice_loss_multiclass
    logits = (rnd(2, 5, 24, 24) * 2).double()
    y = make_target((2, 24, 24), 5)
    for smooth in (0.0, 1.0):
        a, _, _ = dice_ref(logits, y, smooth=smooth)
        assert abs(a.item() - dice_loss_multiclass(logits, y, smooth=smooth).item()) < 1e-12
    xb = (rnd(3, 1, 20, 20) * 3).double()
    yb = torch.randint(0, 2, (3, 1, 20, 20), generator=torch.Generator().manual_seed(2))
    for smooth in (0.0, 1.0):
        a, _, _ = dice_ref(xb, yb, mode="binary", smooth=smooth)
        assert abs(a.item() - dice_loss_binary(xb, yb, smooth=smooth).item()) < 1e-12
    # an ignore_index that does not occur changes nothing; one that does removes exactly those pixels
    assert dice_ref(logits, y, ignore_index=255)[0].item() == dice_ref(logits, y)[0].item()
    yi = y.clone()
    yi[:, :12] = 255
    a, _, _ = dice_ref(logits, yi, ignore_index=255)
    assert abs(a.item() - dice_loss_multiclass(logits[:, :, 12:], y[:, 12:]).item()) < 1e-12


def test_options_struct_matches_the_header():
    """The ctypes mirror of gdl_dice_options has the header's field order."""
    from gdlhip import _lib
    text = (Path(__file__).resolve().parents[1] / "include" / "gdlhip.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} gdl_dice_options;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.strip().split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
    assert [f[0] for f in _lib.DiceOptions._fields_] == fields
    ptr, keep = ops.DiceOptions(-1, 0.5, True, (1, 3)).c_arg()
    o = keep[0]
    assert (o.has_ignore_index, o.ignore_index, o.smooth, o.log_loss, o.num_classes) == (1, -1, 0.5, 1, 2)
    assert [o.classes[i] for i in range(2)] == [1, 3] and ptr


# ------------------------------------------------------------------------------------------------ case 1 and 2: ignore_index
@gpu
@pytest.mark.parametrize("ignore", [255, -1])
def test_ignore_index_full_resolution(ignore):
    B, K, H = 2, 5, 48
    logits = rnd(B, K, H, H) * 2
    y = make_target((B, H, H), K, ignore)
    assert 0.1 < (y == ignore).float().mean().item() < 0.3 and not (y == K - 1).any()
    _, grad = check_full(logits, y, ignore_index=ignore)
    gi = grad.cpu().permute(0, 2, 3, 1)[y == ignore]
    assert gi.numel() > 0 and (gi == 0).all(), "the gradient of an ignored pixel is exactly 0 in every class"
    # an un-squeezed [B, 1, H, W] mask is the same
    a = gnn.DiceLoss(ignore_index=ignore)(logits.to(DEV), y[:, None].to(DEV))
    assert a.item() == gnn.DiceLoss(ignore_index=ignore)(logits.to(DEV), y.to(DEV)).item()


@gpu
@pytest.mark.parametrize("ignore", [255, -1])
def test_ignore_index_binary(ignore):
    B, H = 3, 40
    logits = rnd(B, 1, H, H) * 3
    g = torch.Generator().manual_seed(2)
    y = torch.randint(0, 2, (B, 1, H, H), generator=g)
    y[torch.rand(y.shape, generator=g) < 0.2] = ignore
    _, grad = check_full(logits, y, mode="binary", ignore_index=ignore)
    gi = grad.cpu()[y == ignore]
    assert gi.numel() > 0 and (gi == 0).all()


@gpu
@pytest.mark.parametrize("shape", [(2, 5, 36, 36, 128, 128), (2, 5, 18, 18, 512, 512), (3, 16, 6, 10, 50, 41)])
def test_ignore_index_low_resolution(shape):
    """K <= 8 shapes take the tiled backward, K > 8 the gather kernel; the K <= 8 shapes are also run through the gather
    kernel (gdl_debug_set_dice_lowres_tiled(0)) so that both backward forms are compared on one shape."""
    la, ga, tiles = check_lowres(shape, ignore_index=255)
    assert tiles == (shape[1] <= 8)
    if tiles:
        lb, gb, tiles_b = check_lowres(shape, tiled=False, ignore_index=255)
        assert not tiles_b and torch.equal(la, lb)
        grad_close(ga, gb, f"lowres {shape}: tiled vs gather backward")


@gpu
def test_ignore_index_negative_low_resolution():
    check_lowres((2, 5, 9, 9, 32, 32), ignore_index=-100)


# ------------------------------------------------------------------------------------------------ case 3 and 4
@gpu
@pytest.mark.parametrize("kw", [dict(ignore_index=255), dict(ignore_index=255, smooth=1.0, log_loss=True, classes=[1, 3])],
                         ids=["ignore", "all_options"])
def test_every_pixel_ignored(kw):
    """Loss exactly 0 (no class has a valid pixel), gradient all zeros, nothing NaN -- on the three families."""
    B, K, H = 2, 5, 32
    y = torch.full((B, H, H), 255, dtype=torch.int64, device=DEV)
    ld = (rnd(B, K, H, H) * 2).to(DEV).requires_grad_(True)
    loss = gnn.DiceLoss(**kw)(ld, y)
    (UP * loss).backward()
    assert loss.item() == 0.0 and (ld.grad == 0).all()
    for tiled in (1, 0):
        low = (rnd(B, 9, 9, K) * 2).to(DEV).requires_grad_(True)
        lib = gdlhip._lib.load()
        lib.gdl_debug_set_dice_lowres_tiled(tiled)
        try:
            loss = gnn.DiceLoss(**kw)(gnn.LowresLogits(low, (H, H)), y)
            (UP * loss).backward()
        finally:
            lib.gdl_debug_set_dice_lowres_tiled(1)
        assert loss.item() == 0.0 and (low.grad == 0).all()
    if "classes" not in kw:
        lb = (rnd(B, 1, H, H) * 3).to(DEV).requires_grad_(True)
        loss = gnn.DiceLoss(mode="binary", **kw)(lb, y[:, None])
        (UP * loss).backward()
        assert loss.item() == 0.0 and (lb.grad == 0).all()


@gpu
def test_class_whose_pixels_are_all_ignored_contributes_zero():
    """ignore_index = 3, a real class index: every pixel of class 3 is ignored, so Y_3 = 0 (the masked count) and the class
    contributes 0 although p_3 of the valid pixels is not 0."""
    B, K, H = 2, 5, 40
    logits = rnd(B, K, H, H) * 2
    y = make_target((B, H, H), K, absent=False)
    assert (y == 3).any()
    loss, grad = check_full(logits, y, ignore_index=3)
    _, sums = ops.dice_loss_fwd(logits.to(DEV), y.to(DEV), options=ops.DiceOptions(ignore_index=3))
    assert sums[2 * K + 3].item() == 0.0 and sums[K + 3].item() > 0.0
    assert (grad.cpu().permute(0, 2, 3, 1)[y == 3] == 0).all()
    check_lowres((2, 5, 9, 9, 32, 32), ignore_index=3)


# ------------------------------------------------------------------------------------------------ case 5: smooth, log_loss, classes
OPTION_SETS = [dict(smooth=1.0), dict(log_loss=True), dict(classes=[1, 3]),
               dict(ignore_index=255, smooth=1.0, log_loss=True, classes=[1, 3])]
OPTION_IDS = ["smooth", "log_loss", "classes", "all"]


@gpu
@pytest.mark.parametrize("kw", OPTION_SETS, ids=OPTION_IDS)
def test_options_full_resolution(kw):
    B, K, H = 2, 5, 48
    logits = rnd(B, K, H, H) * 2
    y = make_target((B, H, H), K, kw.get("ignore_index"))
    loss, _ = check_full(logits, y, **kw)
    if set(kw) == {"smooth"}:      # second anchor: the oracle's formula takes smooth
        from oracle.model import dice_loss_multiclass
        assert abs(loss.item() - dice_loss_multiclass(logits.double(), y, smooth=1.0).item()) <= LOSS_TOL


@gpu
@pytest.mark.parametrize("kw", OPTION_SETS, ids=OPTION_IDS)
@pytest.mark.parametrize("shape", [(2, 5, 36, 36, 128, 128), (3, 16, 6, 10, 50, 41)], ids=["tiled", "gather"])
def test_options_low_resolution(shape, kw):
    check_lowres(shape, **kw)


@gpu
@pytest.mark.parametrize("kw", [dict(smooth=1.0), dict(log_loss=True), dict(smooth=1.0, log_loss=True, ignore_index=255, classes=[0])],
                         ids=["smooth", "log_loss", "all"])
def test_options_binary(kw):
    B, H = 3, 40
    logits = rnd(B, 1, H, H) * 3
    g = torch.Generator().manual_seed(2)
    y = torch.randint(0, 2, (B, 1, H, H), generator=g)
    if "ignore_index" in kw:
        y[torch.rand(y.shape, generator=g) < 0.2] = 255
    loss, _ = check_full(logits, y, mode="binary", **kw)
    if set(kw) == {"smooth"}:
        from oracle.model import dice_loss_binary
        assert abs(loss.item() - dice_loss_binary(logits.double(), y, smooth=1.0).item()) <= LOSS_TOL


# ------------------------------------------------------------------------------------------------ case 6: defaults are bit-identical
@gpu
def test_defaults_are_bit_identical_to_the_plain_entry_points():
    """DiceLoss with the defaults spelled out, and the option entry points with an ignore_index that does not occur, against the
    unchanged ops.dice_loss_* / dice_loss_lowres_* / dice_binary_loss_*: torch.equal on loss, sums and gradients."""
    up = torch.tensor(UP, device=DEV)
    crit_kw = dict(ignore_index=None, smooth=0.0, log_loss=False, classes=None)
    unused = ops.DiceOptions(ignore_index=255)
    # full resolution
    B, K, H = 2, 5, 48
    logits, y = (rnd(B, K, H, H) * 2).to(DEV), make_target((B, H, H), K).to(DEV)
    loss0, sums0 = ops.dice_loss_fwd(logits, y)
    g0 = ops.dice_loss_bwd(logits, y, sums0, up)
    ld = logits.clone().requires_grad_(True)
    loss = gnn.DiceLoss(mode="multiclass", **crit_kw)(ld, y)
    (UP * loss).backward()
    assert torch.equal(loss.detach(), loss0) and torch.equal(ld.grad, g0)
    loss1, sums1 = ops.dice_loss_fwd(logits, y, options=unused)
    assert torch.equal(loss1, loss0) and torch.equal(sums1, sums0)
    assert torch.equal(ops.dice_loss_bwd(logits, y, sums1, up, options=unused), g0)
    acc0, acc1 = torch.ones_like(logits), torch.ones_like(logits)
    ops.dice_loss_bwd(logits, y, sums0, up, out=acc0, accumulate=True)
    ops.dice_loss_bwd(logits, y, sums0, up, out=acc1, accumulate=True, options=unused)
    assert torch.equal(acc0, acc1)
    # low resolution: tiled and gather backward
    for B, K, hi, wi, ho, wo in [(2, 5, 36, 36, 128, 128), (2, 5, 18, 18, 512, 512), (3, 16, 6, 10, 50, 41)]:
        low, y = (rnd(B, hi, wi, K, seed=3) * 2).to(DEV), make_target((B, ho, wo), K, seed=4).to(DEV)
        loss0, sums0 = ops.dice_loss_lowres_fwd(low, y, (ho, wo))
        g0 = ops.dice_loss_lowres_bwd(low, y, (ho, wo), sums0, up)
        a = low.clone().requires_grad_(True)
        loss = gnn.DiceLoss(mode="multiclass", **crit_kw)(gnn.LowresLogits(a, (ho, wo)), y)
        (UP * loss).backward()
        assert torch.equal(loss.detach(), loss0) and torch.equal(a.grad, g0)
        loss1, sums1 = ops.dice_loss_lowres_fwd(low, y, (ho, wo), options=unused)
        assert torch.equal(loss1, loss0) and torch.equal(sums1, sums0)
        assert torch.equal(ops.dice_loss_lowres_bwd(low, y, (ho, wo), sums1, up, options=unused), g0)
    # binary
    logits = (rnd(3, 1, 40, 40) * 3).to(DEV)
    y = torch.randint(0, 2, (3, 1, 40, 40), generator=torch.Generator().manual_seed(2)).to(DEV)
    loss0, sums0 = ops.dice_binary_loss_fwd(logits, y)
    g0 = ops.dice_binary_loss_bwd(logits, y, sums0, up)
    ld = logits.clone().requires_grad_(True)
    loss = gnn.DiceLoss(mode="binary", **crit_kw)(ld, y)
    (UP * loss).backward()
    assert torch.equal(loss.detach(), loss0) and torch.equal(ld.grad, g0)
    loss1, sums1 = ops.dice_binary_loss_fwd(logits, y, options=unused)
    assert torch.equal(loss1, loss0) and torch.equal(sums1, sums0)
    assert torch.equal(ops.dice_binary_loss_bwd(logits, y, sums1, up, options=unused), g0)


# ------------------------------------------------------------------------------------------------ case 7: determinism
@gpu
@pytest.mark.parametrize("shape", [(2, 5, 36, 36, 128, 128), (2, 5, 18, 18, 512, 512), (3, 16, 6, 10, 50, 41)])
def test_low_resolution_ignore_index_is_deterministic(shape):
    B, K, hi, wi, ho, wo = shape
    low, y = (rnd(B, hi, wi, K, seed=3) * 2).to(DEV), make_target((B, ho, wo), K, 255, seed=4).to(DEV)
    opt, up = ops.DiceOptions(ignore_index=255), torch.tensor(UP, device=DEV)
    runs = []
    for _ in range(2):
        loss, sums = ops.dice_loss_lowres_fwd(low, y, (ho, wo), options=opt)
        runs.append((loss, sums, ops.dice_loss_lowres_bwd(low, y, (ho, wo), sums, up, options=opt)))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------ case 8: task level
@gpu
def test_dofa_task_with_ignore_index():
    """SegmentationDOFA (the tiny config of test_hip_tasks.py) with DiceLoss(ignore_index=255) and a mask that contains 255:
    validation_step and training_step give the f64 reference's loss on the materialised logits of the same model, the training
    step still asks the model for low-resolution logits, and the IoU counts of the validation mask leave the 255 pixels out.

    Loss bound: 2e-6 per low-resolution Dice term (weights 1 and 0.4) plus one f32 rounding of their sum.
    IoU counts (gdl_iou_counts, unchanged): the intersection and target counts are taken over the labelled pixels only; the
    prediction count |pred == k| is, as the metric defines it, over every pixel."""
    import oracle
    from geo_deep_learning.models.encoders.dofa_v2 import DOFAv2
    from geo_deep_learning.models.segmentation.dofa import DOFASegmentationModel
    from geo_deep_learning.tasks_with_models.segmentation_dofa import SegmentationDOFA
    tiny = dict(patch_size=14, embed_dim=128, depth=4, num_heads=2, out_indices=[0, 1, 2, 3])
    img, nc, b = 112, 5, 4
    ref = oracle.DOFASegmentationModel("dofa_tiny_test", (img, img), num_classes=nc, _encoder_kwargs=tiny, freeze_layers=["encoder"])
    sd = oracle.procedural_state_dict(ref, 7)
    task = SegmentationDOFA("dofa_base", pretrained=False, image_size=(img, img), num_classes=nc, max_samples=2,
                            loss=gnn.DiceLoss(mode="multiclass", ignore_index=255), freeze_layers=["encoder"],
                            wavelengths=[0.665, 0.549, 0.481])
    task.model = DOFASegmentationModel(DOFAv2(img_size=img, pretrained=False, **tiny), (img, img), num_classes=nc,
                                       pretrained=False, freeze_layers=["encoder"])
    task.configure_model()
    task.model.load_state_dict(sd)
    task = task.to(DEV)

    class _Trainer:
        def __init__(self, training):
            self.training, self.datamodule, self.estimated_stepping_batches = training, None, 100
            self.accumulate_grad_batches, self.max_epochs = 1, 3

    batch = oracle.synthetic_batch(b, 3, img, nc, 7)
    batch["wavelengths"] = batch["wavelengths"].unsqueeze(0).expand(b, -1).contiguous()
    g = torch.Generator().manual_seed(5)
    batch["mask"][torch.rand(batch["mask"].shape, generator=g) < 0.2] = 255
    y = batch["mask"].squeeze(1).long()
    assert (y == 255).any()
    dev = {k: (v.to(DEV) if isinstance(v, torch.Tensor) and k != "wavelengths" else v) for k, v in batch.items()}
    asked = []
    model_forward = task.model.forward

    def spy(*a, **kw):
        asked.append(bool(kw.get("lowres_logits", False)))
        return model_forward(*a, **kw)
    task.model.forward = spy

    def want_loss(outputs):
        lo, la = (dice_ref(t.detach().double().cpu(), y, ignore_index=255)[0].item() for t in (outputs.out, outputs.aux))
        return lo + 0.4 * la
    bound = lambda want: LOSS_TOL_LOWRES * 1.4 + 2.0 ** -23 * abs(want)      # noqa: E731
    # ---- validation
    task.trainer = _Trainer(False)
    task.eval()
    with torch.no_grad():
        y_hat = task.validation_step(dev, 0)
        assert asked == [True]
        want = want_loss(task.model(dev["image"], dev["wavelengths"]))
    got = task.logged["val_loss"].item()
    print(f"val_loss {got:.8f} ref {want:.8f} err {abs(got - want):.3e} bound {bound(want):.3e}")
    assert abs(got - want) <= bound(want)
    counts = ops.iou_counts(y_hat, dev["mask"].squeeze(1).long(), nc).cpu()
    p = y_hat.cpu()
    for c in range(nc):
        labelled = y != 255
        assert torch.equal(counts[:, 0, c], ((p == c) & (y == c) & labelled).flatten(1).sum(1))
        assert torch.equal(counts[:, 2, c], ((y == c) & labelled).flatten(1).sum(1))
        assert torch.equal(counts[:, 1, c], (p == c).flatten(1).sum(1))
    assert int(counts[:, 2].sum()) == int((y != 255).sum())
    # ---- training step (train mode: the device-RNG draws are repeated by re-seeding for the materialised forward)
    asked.clear()
    task.trainer = _Trainer(True)
    task.train()
    torch.manual_seed(123)
    loss = task.training_step(dev, 0)
    loss.backward()
    assert asked == [True], "the training step asks the model for low-resolution logits"
    torch.manual_seed(123)
    with torch.no_grad():
        want = want_loss(task.model(dev["image"], dev["wavelengths"]))
    print(f"train_loss {loss.item():.8f} ref {want:.8f} err {abs(loss.item() - want):.3e} bound {bound(want):.3e}")
    assert torch.isfinite(loss).item() and abs(loss.item() - want) <= bound(want)
    grads = [p_.grad for p_ in task.model.parameters() if p_.grad is not None]
    assert len(grads) > 30 and all(torch.isfinite(g_).all().item() for g_ in grads)
    assert any(g_.abs().max().item() > 0 for g_ in grads)
