"""One-class (binary) segmentation from the heads' low-resolution maps on the GPU: the binary Dice / Jaccard / Tversky / Focal
losses evaluated from ``LowresLogits`` [B, h, w, 1] (gather and tile backward forms), the two mask kernels
(``upsample_threshold`` / ``sigmoid_threshold``), a one-class DOFA task with the path on and off, and a captured step.

References are f64 restatements on the CPU -- ``overlap_ref`` (tests/test_overlap_loss_host.py) and ``focal_ref``
(tests/test_focal_host.py) -- applied to ``F.interpolate(low, size, "bilinear", align_corners=False)``, gradients from torch
autograd.  smp is not installed, so parity with smp itself stays unpinned.  Tolerances are those of tests/test_hip_soft_ce.py:
loss within 1e-6 max(1, |ref|) (2e-6 from low-resolution logits), gradients within 1e-4 max|ref|."""

import functools
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_reference", Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


overlap_ref = _load("test_overlap_loss_host").overlap_ref
focal_ref = _load("test_focal_host").focal_ref

DEV = "cuda"
UP = 0.4          # the upstream factor of the auxiliary head
LOSS_TOL, LOSS_TOL_LOWRES, GRAD_TOL = 1e-6, 2e-6, 1e-4

# (B, hi, wi, ho, wo): an integer factor, non-integer factors, a factor of 64, and 1:1 (gather form only)
SHAPES = [(2, 16, 16, 64, 64), (1, 5, 7, 37, 41), (1, 2, 2, 128, 128), (3, 16, 16, 16, 16)]
# the tile-edge and window cases of the kernel skeletons every low-resolution loss shares (csrc/lowres_tile.h; tiles are 32 x 64):
# one partial tile; remainder tiles of one pixel in each direction at a non-integer ratio; the largest factor; 1:1 in one
# direction only; 1:1 in both (gather form only)
SKELETON_SHAPES = [(2, 4, 4, 8, 8), (2, 5, 7, 33, 65), (2, 1, 1, 64, 64), (2, 8, 8, 8, 16), (2, 8, 8, 8, 8)]

# name -> (class, constructor arguments, the f64 reference of the loss on full-resolution logits [B,1,H,W])
CASES = {
    "dice": (gnn.DiceLoss, dict(mode="binary"), lambda x, y: overlap_ref(x, y, "dice", mode="binary")[0]),
    "dice-options": (gnn.DiceLoss, dict(mode="binary", smooth=1.0, log_loss=True, ignore_index=255),
                     lambda x, y: overlap_ref(x, y, "dice", mode="binary", smooth=1.0, log_loss=True, ignore_index=255)[0]),
    "jaccard": (gnn.JaccardLoss, dict(mode="binary"), lambda x, y: overlap_ref(x, y, "jaccard", mode="binary")[0]),
    "tversky": (gnn.TverskyLoss, dict(mode="binary", alpha=0.3, beta=0.7, gamma=0.75, ignore_index=-1),
                lambda x, y: overlap_ref(x, y, "tversky", mode="binary", alpha=0.3, beta=0.7, gamma=0.75, ignore_index=-1)[0]),
}
CASES["focal-noignore"] = (gnn.FocalLoss, dict(mode="binary", alpha=0.25, gamma=2.0),
                           lambda x, y: focal_ref(x, y, mode="binary", alpha=0.25, gamma=2.0))
for _g in (0.0, 0.5, 2.0):
    for _r in ("mean", "sum"):
        CASES[f"focal-g{_g}-{_r}"] = (
            gnn.FocalLoss, dict(mode="binary", alpha=0.25, gamma=_g, ignore_index=255, reduction=_r),
            functools.partial(lambda x, y, g, r: focal_ref(x, y, mode="binary", alpha=0.25, gamma=g, ignore_index=255, reduction=r),
                              g=_g, r=_r))


def forms_of(shape):
    B, hi, wi, ho, wo = shape
    tiles = gdlhip._lib.load().gdl_binary_lowres_bwd_workspace(B, hi, wi, ho, wo) > 0
    assert tiles == ((hi, wi) != (ho, wo)), "every shape here but the 1:1 one takes the tile form"
    return ("tile", "gather") if tiles else ("gather",)


def make_inputs(shape, ignore, seed=0):
    """low [B,hi,wi,1] (randn * 2) and a 0/1 target; with ``ignore``: 10 % of the pixels at random plus the top-left ninth of
    image 0 (so that some low-resolution logits have every contributing pixel ignored).  SKELETON_SHAPES: a quarter of the pixels
    at random plus the whole first 32 x 64 tile of image 0."""
    B, hi, wi, ho, wo = shape
    g = torch.Generator().manual_seed(seed + sum(shape))
    low = torch.randn(B, hi, wi, 1, generator=g) * 2.0
    tgt = torch.randint(0, 2, (B, ho, wo), generator=g)
    if ignore is not None and shape in SKELETON_SHAPES:
        tgt[torch.rand(tgt.shape, generator=g) < 0.25] = ignore
        tgt[0, :32, :64] = ignore
    elif ignore is not None:
        tgt[torch.rand(tgt.shape, generator=g) < 0.1] = ignore
        tgt[0, : ho // 3, : wo // 3] = ignore
        share = (tgt == ignore).float().mean().item()
        assert 0.10 <= share <= 0.30, share
    return low, tgt


@functools.lru_cache(maxsize=None)
def reference(shape, case):
    """(low, target, f64 loss, UP * d loss / d low [B,hi,wi,1], dead): computed once per shape and case, never modified.  ``dead``
    marks the low-resolution logits whose every contributing pixel is ignored (from the resize's own weights)."""
    _, kw, ref_fn = CASES[case]
    ignore = kw.get("ignore_index")
    low, tgt = make_inputs(shape, ignore)
    size = shape[3:]
    lr = low.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = ref_fn(F.interpolate(lr, size=size, mode="bilinear", align_corners=False), tgt)
    (UP * ref).backward()
    dead = torch.zeros_like(low, dtype=torch.bool)
    if ignore is not None:
        w = low.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        valid = (tgt != ignore).double()[:, None]
        (F.interpolate(w, size=size, mode="bilinear", align_corners=False) * valid).sum().backward()
        dead = (w.grad == 0).permute(0, 2, 3, 1)
    return low, tgt, ref.item(), lr.grad.permute(0, 2, 3, 1).contiguous(), dead


def loss_close(got, ref, tol, what):
    err, bound = abs(got - ref), tol * max(1.0, abs(ref))
    print(f"{what}: loss {got:.8f} ref {ref:.8f} err {err:.3e} bound {bound:.3e}")
    assert err <= bound, f"{what}: loss {got:.8f} ref {ref:.8f} err {err:.3e} bound {bound:.3e}"


def grad_close(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    s = max(ref.abs().max().item(), 1e-12)
    err = (got - ref).abs().max().item()
    print(f"{what}: grad max err {err:.3e} vs scale {s:.3e}")
    assert err <= GRAD_TOL * s, f"{what}: grad max err {err:.3e} vs scale {s:.3e}"


def run_ops(crit, low, tgt, size, form, up=UP):
    """(loss, d low) through the op wrappers with the backward form ``form``."""
    upt = torch.tensor(up, device=DEV)
    if isinstance(crit, gnn.FocalLoss):
        loss, norm = ops.focal_binary_lowres_fwd(low, tgt, size, crit.options)
        return loss, ops.focal_binary_lowres_bwd(low, tgt, size, norm, upt, 1.0, crit.options, form=form)
    loss, sums = ops.dice_binary_lowres_fwd(low, tgt, size, crit.eps, options=crit.options)
    return loss, ops.dice_binary_lowres_bwd(low, tgt, size, sums, upt, 1.0, crit.eps, options=crit.options, form=form)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("shape", SHAPES + SKELETON_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradient_from_the_low_resolution_map(shape, case):
    """Every backward form the shape admits, against the f64 reference and against the class's own materialised path; the class
    itself takes the low-resolution node (``upsample_logits`` is never called) and its first form, up to the factor at which that
    is the faster route."""
    cls, kw, _ = CASES[case]
    low, tgt, ref_loss, ref_grad, dead = reference(shape, case)
    size = tuple(shape[3:])
    crit = cls(**kw)
    lowd, tgtd = low.to(DEV), tgt.to(DEV)
    b_ = lowd.clone().requires_grad_(True)
    lb = crit(gnn.LowresLogits(b_, size).materialise(), tgtd)
    (UP * lb).backward()
    forms = forms_of(shape)
    got = {}
    for form in forms:
        what = f"{case} {shape} {form}"
        loss, grad = run_ops(crit, lowd, tgtd, size, form)
        assert loss.dim() == 0 and torch.isfinite(loss).item() and torch.isfinite(grad).all().item()
        loss_close(loss.item(), ref_loss, LOSS_TOL_LOWRES, what)
        loss_close(loss.item(), lb.item(), LOSS_TOL, what + " vs the materialised path")
        grad_close(grad, ref_grad, what + " vs torch")
        grad_close(grad, b_.grad, what + " vs the materialised path")
        if dead.any():
            assert (grad.cpu()[dead] == 0).all(), what + ": a logit whose every contributing pixel is ignored gets exactly 0"
        got[form] = (loss, grad)
    if kw.get("ignore_index") is not None and shape[1] >= 5:
        assert dead.any()
    for form in forms[:-1]:
        assert torch.equal(got[form][0], got["gather"][0]), "the forms share the forward"
        grad_close(got[form][1], got["gather"][1], f"{case} {shape} {form} vs gather")
    calls = []
    real = ops.upsample_logits
    ops.upsample_logits = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        a = lowd.clone().requires_grad_(True)
        la = crit(gnn.LowresLogits(a, size), tgtd)
        (UP * la).backward()
    finally:
        ops.upsample_logits = real
    if ops.binary_lowres_pays(lowd, size):
        assert calls == [], "the class reads the low-resolution map"
        assert torch.equal(la.detach(), got[forms[0]][0]) and torch.equal(a.grad, got[forms[0]][1])
    else:      # a factor at which materialising was measured to be faster: the class takes that route
        assert calls == [1] and torch.equal(la.detach(), lb.detach()) and torch.equal(a.grad, b_.grad)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_all_negative_and_all_ignored_targets(shape):
    """Dice family, no positive pixel: loss 0 and a finite, all-zero gradient.  Every loss with an ignore_index, every pixel
    ignored: the same.

    FocalLoss on an all-negative target is NOT asserted to be 0, on purpose: focal loss sums -(1 - alpha) p^gamma log(1 - p)
    over the negative pixels, which is positive for every finite logit, so "loss 0, zero gradient" holds for the Dice family
    only (smp zeroes a class without positives there) and for no correct focal kernel.  That case is checked against the f64
    reference instead: loss and gradient within the tolerances of this file, both finite."""
    B, hi, wi, ho, wo = shape
    size = (ho, wo)
    low_cpu = make_inputs(shape, None, seed=5)[0]
    low = low_cpu.to(DEV)
    negative = torch.zeros(B, ho, wo, dtype=torch.int64)
    for case, (cls, kw, ref_fn) in CASES.items():
        crit = cls(**kw)
        if isinstance(crit, gnn.FocalLoss):
            lr = low_cpu.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
            ref = ref_fn(F.interpolate(lr, size=size, mode="bilinear", align_corners=False), negative)
            (UP * ref).backward()
            assert ref.item() > 0
            for form in forms_of(shape):
                what = f"{case} {shape} {form} all-negative"
                loss, grad = run_ops(crit, low, negative.to(DEV), size, form)
                assert torch.isfinite(loss).item() and torch.isfinite(grad).all().item(), what
                loss_close(loss.item(), ref.item(), LOSS_TOL_LOWRES, what)
                grad_close(grad, lr.grad.permute(0, 2, 3, 1), what)
        targets = []
        if not isinstance(crit, gnn.FocalLoss):
            targets.append(("all-negative", negative.to(DEV)))
        if kw.get("ignore_index") is not None:
            targets.append(("all-ignored", torch.full((B, ho, wo), kw["ignore_index"], dtype=torch.int64, device=DEV)))
        for name, tgt in targets:
            for form in forms_of(shape):
                loss, grad = run_ops(crit, low, tgt, size, form)
                assert loss.item() == 0.0 and torch.isfinite(grad).all().item() and (grad == 0).all().item(), (case, name, form)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_two_launches_give_the_same_bits(shape):
    for case in ("dice", "tversky", "focal-g2.0-mean"):
        cls, kw, _ = CASES[case]
        low, tgt = (t.to(DEV) for t in reference(shape, case)[:2])
        for form in forms_of(shape):
            runs = [run_ops(cls(**kw), low, tgt, tuple(shape[3:]), form) for _ in range(2)]
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), (case, shape, form)


def test_c_entry_points_refuse_shapes_outside_the_limits():
    """A downsample, a factor above 64 and the tile form on a 1:1 map are GDL_CHECK_ARG errors (status -1), not fallbacks."""
    lib = gdlhip._lib.load()
    P = ops._p
    low, y = torch.zeros(1, 8, 8, 1, device=DEV), torch.zeros(1, 8, 8, dtype=torch.int64, device=DEV)
    sums, loss, ws = torch.zeros(3, device=DEV), torch.zeros((), device=DEV), torch.zeros(4096, device=DEV)
    norm = torch.ones(1, device=DEV)
    mask = torch.zeros(1, 8, 8, dtype=torch.int64, device=DEV)
    fopt = ops.FocalOptions().c_args()
    for hi, wi, ho, wo in ((8, 8, 4, 8), (8, 8, 8, 4), (1, 1, 65, 8), (1, 1, 8, 65)):
        assert lib.gdl_dice_binary_loss_lowres_fwd(P(low), P(y), 1, hi, wi, ho, wo, 1e-7, P(sums), P(loss), P(ws), 16384, None) == -1
        assert lib.gdl_dice_binary_loss_lowres_bwd(P(low), P(y), 1, hi, wi, ho, wo, 1e-7, P(sums), None, 1.0, P(low), P(ws), 16384, 0, None) == -1
        assert lib.gdl_focal_binary_lowres_fwd(P(low), P(y), 1, hi, wi, ho, wo, *fopt, P(loss), P(norm), P(ws), 16384, None) == -1
        assert lib.gdl_focal_binary_lowres_bwd(P(low), P(y), 1, hi, wi, ho, wo, *fopt, P(norm), None, 1.0, P(low), P(ws), 16384, 0, None) == -1
        assert lib.gdl_upsample_threshold(P(low), 1, hi, wi, P(mask), ho, wo, 0.5, None) == -1
    with pytest.raises(ValueError, match="tile form"):
        ops.dice_binary_lowres_bwd(low, y, (8, 8), sums, None, form="tile")
    with pytest.raises(ValueError, match="tile form"):
        ops.focal_binary_lowres_bwd(low, y, (8, 8), norm, None, form="tile")


# ------------------------------------------------------------------------------------------------ the mask kernels
def _mask_reference(x, th):
    """The torch expression on materialised logits ``x`` [B,1,H,W] (CPU), and the pixels within 1e-6 of the threshold (f64)."""
    ref = (x.sigmoid().squeeze(1) > th).long()
    near = ((x.double().sigmoid() - th).abs() < 1e-6).squeeze(1)
    return ref, near


@pytest.mark.parametrize("th", [0.5, 0.3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_threshold_is_the_threshold_of_the_materialised_logits(shape, th):
    B, hi, wi, ho, wo = shape
    low = (torch.randn(B, hi, wi, 1, generator=torch.Generator().manual_seed(11 + sum(shape))) * 2).to(DEV)
    mat = gnn.LowresLogits(low, (ho, wo)).materialise()
    a, b = ops.upsample_threshold(low, (ho, wo), th), ops.sigmoid_threshold(mat, th)
    assert a.dtype == torch.int64 and a.shape == (B, ho, wo) and b.shape == (B, ho, wo)
    assert torch.equal(a, b), "one kernel or two: the same mask in every pixel"
    assert torch.equal(gnn.predict_binary_mask(gnn.LowresLogits(low, (ho, wo)), th), a) and torch.equal(gnn.predict_binary_mask(mat, th), a)
    ref, near = _mask_reference(mat.cpu(), th)
    share = near.float().mean().item()
    print(f"{shape} th={th}: {near.sum().item()} of {near.numel()} pixels within 1e-6 of the threshold; ones: {ref.float().mean().item():.3f}")
    assert share <= 1e-3, "asserted from the reference alone"
    if hi >= 5:      # (four logits can all lie on one side)
        assert 0.05 < ref.float().mean().item() < 0.95
    assert torch.equal(a.cpu()[~near], ref[~near]) and torch.equal(b.cpu()[~near], ref[~near])


def test_exact_threshold_values_compare_in_probability_space():
    """A map quantised to multiples of 0.5: at 1:1 the resize is the identity and at factor 4 every interpolated value is a
    multiple of 1 / 128, so 0 occurs exactly and nothing else is near it.  Hand-computed: sigmoid(0) > 0.5 is False, so the mask
    is [x > 0].  Logits of 1e-8 are positive, but their f32 sigmoid is exactly 0.5: 0 as well, as in the reference's expression."""
    g = torch.Generator().manual_seed(3)
    for B, hi, wi, ho, wo in ((3, 16, 16, 16, 16), (2, 16, 16, 64, 64)):
        low = (torch.randint(-2, 3, (B, hi, wi, 1), generator=g).float() * 0.5).to(DEV)
        mat = gnn.LowresLogits(low, (ho, wo)).materialise()
        x = mat.cpu().squeeze(1)
        assert (x == 0).sum().item() > 10 and ((x != 0) & (x.abs() < 1 / 256)).sum().item() == 0
        want = (x > 0).long()
        assert torch.equal(want, (mat.cpu().sigmoid().squeeze(1) > 0.5).long())
        assert torch.equal(ops.upsample_threshold(low, (ho, wo), 0.5).cpu(), want)
        assert torch.equal(ops.sigmoid_threshold(mat, 0.5).cpu(), want)
    flat = torch.tensor([0.0, 1e-8, -1e-8, 1e-5, -1e-5, 3.0, -3.0], device=DEV)
    assert ops.sigmoid_threshold(flat, 0.5).tolist() == [0, 0, 0, 1, 0, 1, 0]
    assert ops.sigmoid_threshold(flat, 0.3).tolist() == [1, 1, 1, 1, 1, 1, 0]


# ------------------------------------------------------------------------------------------------ task level
IMG = 32


def _one_class_dofa_task(loss):
    """The tiny DOFA task of tests/test_hip_soft_ce.py with ``num_classes: 1`` and 4 x 4 patches on 3 x 32 x 32 images (frozen
    encoder): the main head's map is 32 x 32 (1:1, the gather form) and the auxiliary head's 4 x 4 (factor 8, the tile form), both
    inside the range the binary losses read from the low-resolution map (ops.BINARY_LOWRES_MAX_FACTOR).  DOFA-base at 512 x 512 has
    factors 4 and 32: there the auxiliary head is beyond that range and is materialised, which was measured to be faster."""
    import oracle
    from geo_deep_learning.models.encoders.dofa_v2 import DOFAv2
    from geo_deep_learning.models.segmentation.dofa import DOFASegmentationModel
    from geo_deep_learning.tasks_with_models.segmentation_dofa import SegmentationDOFA
    tiny = dict(patch_size=4, embed_dim=128, depth=4, num_heads=2, out_indices=[0, 1, 2, 3])
    img = IMG
    ref = oracle.DOFASegmentationModel("dofa_tiny_test", (img, img), num_classes=1, _encoder_kwargs=tiny, freeze_layers=["encoder"])
    sd = oracle.procedural_state_dict(ref, 7)
    task = SegmentationDOFA("dofa_base", pretrained=False, image_size=(img, img), num_classes=1, max_samples=2, loss=loss,
                            freeze_layers=["encoder"], wavelengths=[0.665, 0.549, 0.481])
    task.model = DOFASegmentationModel(DOFAv2(img_size=img, pretrained=False, **tiny), (img, img), num_classes=1,
                                       pretrained=False, freeze_layers=["encoder"])
    task.configure_model()
    task.model.load_state_dict(sd)
    task = task.to(DEV)

    class _Trainer:
        training, datamodule, estimated_stepping_batches, accumulate_grad_batches, max_epochs = True, None, 100, 1, 3
    task.trainer = _Trainer()
    return task


def _one_class_batch(seed, b=4):
    import oracle
    batch = oracle.synthetic_batch(b, 3, IMG, 2, seed)
    batch["wavelengths"] = batch["wavelengths"].unsqueeze(0).expand(b, -1).contiguous()
    batch["mask"] = batch["mask"].long()
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) and k != "wavelengths" else v) for k, v in batch.items()}


@pytest.mark.parametrize("loss", [gnn.DiceLoss(mode="binary"), gnn.FocalLoss("binary", alpha=0.25, ignore_index=255)], ids=["dice", "focal"])
def test_one_class_dofa_task_with_the_path_on_and_off(monkeypatch, loss):
    """``training_step`` and ``validation_step`` of a one-class DOFA task give the same loss (1e-6) and the same mask with
    GDL_LOWRES_DICE on and off, and the on-run never calls ``upsample_logits``."""
    task = _one_class_dofa_task(loss)
    batch = _one_class_batch(7)
    if isinstance(loss, gnn.FocalLoss):
        g = torch.Generator().manual_seed(5)
        batch["mask"][(torch.rand(batch["mask"].shape, generator=g) < 0.2).to(DEV)] = 255
    logged = {}
    task.log = lambda name, value, **kw: logged.__setitem__(name, value)
    calls = []
    real = ops.upsample_logits
    monkeypatch.setattr(ops, "upsample_logits", lambda *a, **k: calls.append(1) or real(*a, **k))
    out = {True: [], False: []}
    task.train()
    for on in (True, False):
        monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", on)
        calls.clear()
        task.zero_grad(set_to_none=True)
        torch.manual_seed(123)
        lt = task.training_step(batch, 0)
        lt.backward()
        out[on] += [lt.item(), None, None, {n: p.grad.clone() for n, p in task.model.named_parameters() if p.grad is not None}, len(calls)]
    task.eval()      # (after both training steps: they move the BatchNorm running statistics the validation reads)
    for on in (True, False):
        monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", on)
        calls.clear()
        with torch.no_grad():
            out[on][2] = task.validation_step(batch, 0)
        out[on][1] = logged["val_loss"].item()
        out[on][4] += len(calls)
    print(f"train loss on {out[True][0]:.8f} off {out[False][0]:.8f}; val loss on {out[True][1]:.8f} off {out[False][1]:.8f}; "
          f"upsample_logits calls on {out[True][4]} off {out[False][4]}")
    assert out[True][4] == 0 and out[False][4] == 4, "two heads, training and validation"
    assert abs(out[True][0] - out[False][0]) <= 1e-6 and abs(out[True][1] - out[False][1]) <= 1e-6
    assert out[True][2].dtype == torch.int64 and out[True][2].shape == (4, IMG, IMG)
    assert torch.equal(out[True][2], out[False][2])
    print(f"share of ones in the mask: {out[True][2].float().mean().item():.4f}")
    assert len(out[True][3]) > 30 and out[True][3].keys() == out[False][3].keys()
    for n, ga in out[True][3].items():      # the bounds tests/test_hip_soft_ce.py holds the same comparison to
        gb = out[False][3][n]
        err, rn = (ga - gb).norm().item(), gb.norm().item()
        assert err <= 3e-2 * rn + 2e-6, (n, err, rn)
    assert any(g_.abs().max().item() > 0 for g_ in out[True][3].values())


def test_graphed_binary_dice_step_reproduces_the_eager_losses_bit_for_bit():
    """GraphedTrainStep (hipGraph capture of forward + DiceLoss(binary) from the one-class low-resolution maps + backward + Adam):
    one capture and two replays against the same steps run eagerly, bit for bit.  In a fresh child process
    (tests/_loss_graph_worker.py, scenario "binary_lowres") under its own time limit, one capture scenario per process."""
    worker = Path(__file__).with_name("_loss_graph_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(worker), "binary_lowres"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    print(res)
    assert len(res["eager"]) == 2 and res["eager"] == res["graphed"], res
    assert res["upsample_logits_calls"] == 0
