"""gdlhip.nn.JaccardLoss and TverskyLoss on the GPU: the full-resolution, binary and low-resolution (LowresLogits) families,
forward and backward, against ``overlap_ref`` of test_overlap_loss_host.py -- the formulas restated with plain torch ops,
evaluated in f64 on the CPU, gradients from autograd.  Nothing here is compared against the kernels' own output except where a
test is about two paths of the kernels agreeing (low-resolution vs materialised, determinism, Dice unchanged).

Tolerances are those test_hip_dice_options.py applies to the Dice option kernels (the same three sums, the same f32 pixel
passes), imported from there unchanged: loss within 1e-6 of the f64 reference (2e-6 from low-resolution logits), divided by the
smallest ``score_k`` of a present, selected class with ``log_loss`` (its ``loss_bound``); gradients within 1e-4 of max|ref|.
The focal exponent ``gamma`` gets no allowance of its own.

Inputs are random logits, so the class mean ``m`` stays far from 0 and the ``m <= 0`` rule is never part of a tolerance
comparison; ``test_perfect_prediction_has_a_zero_gradient`` covers that rule with an exact check."""

import pytest
import torch
import torch.nn.functional as F

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402
from test_hip_dice_options import GRAD_TOL, LOSS_TOL, LOSS_TOL_LOWRES, UP, grad_close, loss_bound, make_target  # noqa: E402
from test_overlap_loss_host import overlap_ref  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda"

JACCARD = [dict(), dict(smooth=1.0), dict(log_loss=True), dict(classes=[1, 3])]
TVERSKY = [dict(alpha=0.3, beta=0.7), dict(alpha=0.7, beta=0.3, gamma=0.75), dict(gamma=2.0, smooth=1.0),
           dict(ignore_index=255), dict(log_loss=True, classes=[0, 2])]
GRID = [("jaccard", kw) for kw in JACCARD] + [("tversky", kw) for kw in TVERSKY]
GRID_IDS = ["jaccard-default", "jaccard-smooth", "jaccard-log", "jaccard-classes", "tversky-a3b7", "tversky-a7b3-g075",
            "tversky-g2-smooth", "tversky-ignore", "tversky-log-classes"]
# low [B, h, w, K] -> (H, W).  K <= 8 takes the tiled backward, K > 8 the gather kernel (dice_tile_dims in csrc/loss_dice.hip: the
# two tile-extent conditions always hold for an upsample, so the class count alone decides): K = 8 and K = 9 are the smallest
# change of shape across that condition.
LOWRES = [(2, 4, 4, 5, 32, 32), (2, 2, 2, 5, 64, 64), (2, 3, 5, 3, 24, 40), (2, 3, 4, 8, 9, 10), (2, 3, 4, 9, 9, 10)]
LOWRES_IDS = ["x8", "x32", "nonsquare", "K8-tiled", "K9-gather"]
# the tile-edge and window cases of tests/test_hip_soft_ce.py::SKELETON_SIZES, at the class counts 5, 8 (the tile limit), 9 and 16
EDGES = [(2, hi, wi, K, ho, wo) for hi, wi, ho, wo in [(4, 4, 8, 8), (5, 7, 33, 65), (1, 1, 64, 64), (8, 8, 8, 16), (8, 8, 8, 8)]
         for K in (5, 8, 9, 16)]


def make(kind, mode="multiclass", **kw):
    return (gnn.JaccardLoss if kind == "jaccard" else gnn.TverskyLoss)(mode=mode, **kw)


def uniform(*shape, scale=4.0, seed=0):
    """Logits spread over +-scale."""
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed + sum(shape))) * 2.0 - 1.0) * scale


def fits(kw, k):
    return kw.get("classes") is None or max(kw["classes"]) < k


def check_full(kind, logits, target, mode="multiclass", **kw):
    x = logits.double().clone().requires_grad_(True)
    ref, score, ysum, m = overlap_ref(x, target, kind, mode, **kw)
    assert m.item() > 0.05, "inputs keep the class mean away from 0"
    (UP * ref).backward()
    ld = logits.to(DEV).requires_grad_(True)
    loss = make(kind, mode, **kw)(ld, target.to(DEV))
    (UP * loss).backward()
    bound = loss_bound(LOSS_TOL, kw, score, ysum)
    err = abs(loss.item() - ref.item())
    print(f"{kind} {mode} {tuple(logits.shape)} {kw}: loss {loss.item():.8f} ref {ref.item():.8f} err {err:.3e} bound {bound:.3e}")
    assert torch.isfinite(loss).item() and torch.isfinite(ld.grad).all().item()
    assert err <= bound
    grad_close(ld.grad, x.grad, f"{kind} {mode} {kw}")
    return loss, ld.grad


def check_lowres(kind, shape, tile_ignored=False, **kw):
    """On LowresLogits: against overlap_ref on the interpolated logits, and against the same loss on materialise()d logits.
    ``tile_ignored``: the whole first 32 x 64 tile of image 0 is ignored on top of the random quarter."""
    B, hi, wi, K, ho, wo = shape
    low = uniform(B, hi, wi, K, seed=3)
    tgt = make_target((B, ho, wo), K, kw.get("ignore_index"), frac=0.25, seed=4)
    if tile_ignored:
        tgt[0, :32, :64] = kw["ignore_index"]
    lr = low.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref, score, ysum, m = overlap_ref(F.interpolate(lr, size=(ho, wo), mode="bilinear", align_corners=False), tgt, kind, **kw)
    assert m.item() > 0.05
    (UP * ref).backward()
    lowd, tgtd = low.to(DEV), tgt.to(DEV)
    crit = make(kind, **kw)
    a = lowd.clone().requires_grad_(True)
    b_ = lowd.clone().requires_grad_(True)
    tiles = gdlhip._lib.load().gdl_dice_loss_lowres_bwd_workspace(B, K, hi, wi, ho, wo) > 0
    la = crit(gnn.LowresLogits(a, (ho, wo)), tgtd)
    (UP * la).backward()
    lb = crit(gnn.LowresLogits(b_, (ho, wo)).materialise(), tgtd)
    (UP * lb).backward()
    bound = loss_bound(LOSS_TOL_LOWRES, kw, score, ysum)
    err = abs(la.item() - ref.item())
    print(f"{kind} lowres {shape} tiled={tiles} {kw}: loss {la.item():.8f} ref {ref.item():.8f} err {err:.3e} bound {bound:.3e}; "
          f"vs materialised {abs(la.item() - lb.item()):.3e}")
    assert torch.isfinite(la).item() and torch.isfinite(a.grad).all().item()
    assert err <= bound
    assert abs(la.item() - lb.item()) <= loss_bound(LOSS_TOL, kw, score, ysum)
    grad_close(a.grad.permute(0, 3, 1, 2), lr.grad, f"{kind} lowres {shape} {kw} vs torch")
    grad_close(a.grad, b_.grad, f"{kind} lowres {shape} {kw} vs the materialised path")
    return tiles


# ------------------------------------------------------------------------------------------------ full resolution, multiclass
@gpu
@pytest.mark.parametrize("kind,kw", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("shape", [(2, 5, 32, 32), (2, 3, 24, 40)], ids=["K5", "K3"])
def test_full_resolution(shape, kind, kw):
    B, K, H, W = shape
    logits = uniform(*shape)
    ign = kw.get("ignore_index")
    y = make_target((B, H, W), K, ign, frac=0.25)
    assert not (y == K - 1).any(), "one class is absent from the target"
    if not fits(kw, K):      # class 3 of 3: the case cannot be formed on this shape; the range check must say so
        with pytest.raises(ValueError, match="out of range"):
            make(kind, **kw)(logits.to(DEV), y.to(DEV))
        return
    loss, grad = check_full(kind, logits, y, **kw)
    if ign is not None:
        assert 0.15 < (y == ign).float().mean().item() < 0.35
        gi = grad.cpu().permute(0, 2, 3, 1)[y == ign]
        assert gi.numel() > 0 and (gi == 0).all(), "the gradient of an ignored pixel is exactly 0 in every class"
    # an un-squeezed [B, 1, H, W] mask is the same
    assert make(kind, **kw)(logits.to(DEV), y[:, None].to(DEV)).item() == loss.item()


# ------------------------------------------------------------------------------------------------ binary
@gpu
@pytest.mark.parametrize("kind,kw", GRID, ids=GRID_IDS)
def test_binary(kind, kw):
    kw = dict(kw)
    if "classes" in kw:
        kw["classes"] = [0]          # the single class of binary mode
    logits = uniform(2, 1, 32, 32)
    g = torch.Generator().manual_seed(2)
    y = torch.randint(0, 2, (2, 1, 32, 32), generator=g)
    ign = kw.get("ignore_index")
    if ign is not None:
        y[torch.rand(y.shape, generator=g) < 0.25] = ign
    _, grad = check_full(kind, logits, y, mode="binary", **kw)
    if ign is not None:
        gi = grad.cpu()[y == ign]
        assert gi.numel() > 0 and (gi == 0).all()


# ------------------------------------------------------------------------------------------------ low resolution
@gpu
@pytest.mark.parametrize("kind,kw", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("shape", LOWRES, ids=LOWRES_IDS)
def test_low_resolution(shape, kind, kw):
    K = shape[3]
    if not fits(kw, K):
        low = uniform(shape[0], shape[1], shape[2], K).to(DEV)
        y = torch.zeros(shape[0], shape[4], shape[5], dtype=torch.int64, device=DEV)
        with pytest.raises(ValueError, match="out of range"):
            make(kind, **kw)(gnn.LowresLogits(low, shape[4:]), y)
        return
    assert check_lowres(kind, shape, **kw) == (K <= 8), "K <= 8 runs the tiled backward, K > 8 the gather kernel"


@gpu
@pytest.mark.parametrize("ignore", [255, None], ids=["ignored", "none_ignored"])
@pytest.mark.parametrize("shape", EDGES, ids=lambda s: "x".join(map(str, s)))
def test_low_resolution_at_the_tile_edges(shape, ignore):
    kw = dict(alpha=0.3, beta=0.7, smooth=1.0, ignore_index=ignore)
    assert check_lowres("tversky", shape, tile_ignored=ignore is not None, **kw) == (shape[3] <= 8)


# ------------------------------------------------------------------------------------------------ ignored pixels
@gpu
@pytest.mark.parametrize("kw", [dict(ignore_index=255), dict(ignore_index=255, alpha=0.3, beta=0.7, gamma=0.75, smooth=1.0)],
                         ids=["ignore", "focal"])
def test_every_pixel_ignored(kw):
    """Loss exactly 0 (no class has a valid pixel, so m = 0), gradient all zeros, nothing NaN -- on every family."""
    B, H = 2, 32
    y = torch.full((B, H, H), 255, dtype=torch.int64, device=DEV)
    ld = uniform(B, 5, H, H).to(DEV).requires_grad_(True)
    loss = gnn.TverskyLoss(**kw)(ld, y)
    (UP * loss).backward()
    assert loss.item() == 0.0 and (ld.grad == 0).all()
    for K in (5, 9):      # tiled and gather backward
        low = uniform(B, 4, 4, K).to(DEV).requires_grad_(True)
        loss = gnn.TverskyLoss(**kw)(gnn.LowresLogits(low, (H, H)), y)
        (UP * loss).backward()
        assert loss.item() == 0.0 and (low.grad == 0).all()
    lb = uniform(B, 1, H, H).to(DEV).requires_grad_(True)
    loss = gnn.TverskyLoss(mode="binary", **kw)(lb, y[:, None])
    (UP * loss).backward()
    assert loss.item() == 0.0 and (lb.grad == 0).all()


# ------------------------------------------------------------------------------------------------ the m <= 0 rule
@gpu
@pytest.mark.parametrize("log_loss", [False, True], ids=["plain", "log"])
def test_perfect_prediction_has_a_zero_gradient(log_loss):
    """Target = arg-max of +-30 logits, the mean over the present classes only: every p is 0 or 1 in f32, so score_k = 1 and
    m = 0 exactly.  With gamma = 0.75 torch's gamma * m ** (gamma - 1) is inf (and inf * 0 = nan in the chain); the documented
    rule makes the factor 0: loss exactly 0, gradient finite and exactly 0."""
    B, K, H = 2, 5, 16
    y = make_target((B, H, H), K)                 # classes 0..3 present, class 4 absent
    logits = (F.one_hot(y, K).permute(0, 3, 1, 2).float() * 60.0 - 30.0).contiguous()
    ref = overlap_ref(logits.double().requires_grad_(True), y, "tversky", classes=[0, 1, 2, 3], gamma=0.75, log_loss=log_loss)
    assert ref[3].item() <= 1e-20, "the restatement's m is 0 up to exp(-60)"
    ld = logits.to(DEV).requires_grad_(True)
    loss = gnn.TverskyLoss(classes=[0, 1, 2, 3], alpha=0.3, beta=0.7, gamma=0.75, log_loss=log_loss)(ld, y.to(DEV))
    (UP * loss).backward()
    assert loss.item() == 0.0
    assert torch.isfinite(ld.grad).all().item() and (ld.grad == 0).all()
    low = ld.detach().permute(0, 2, 3, 1).contiguous().requires_grad_(True)      # a 1:1 "resize": the same pixels
    loss = gnn.TverskyLoss(classes=[0, 1, 2, 3], gamma=0.75, log_loss=log_loss)(gnn.LowresLogits(low, (H, H)), y.to(DEV))
    (UP * loss).backward()
    assert loss.item() == 0.0 and torch.isfinite(low.grad).all().item() and (low.grad == 0).all()


# ------------------------------------------------------------------------------------------------ determinism
@gpu
@pytest.mark.parametrize("shape", [LOWRES[0], LOWRES[4]], ids=["tiled", "gather"])
def test_low_resolution_is_deterministic(shape):
    B, hi, wi, K, ho, wo = shape
    low, y = uniform(B, hi, wi, K, seed=3).to(DEV), make_target((B, ho, wo), K, 255, frac=0.25, seed=4).to(DEV)
    up = torch.tensor(UP, device=DEV)
    for opt in (ops.OverlapOptions("tversky", 255, 1.0, False, None, 0.3, 0.7, 0.75), ops.OverlapOptions("jaccard")):
        runs = []
        for _ in range(2):
            loss, sums = ops.dice_loss_lowres_fwd(low, y, (ho, wo), options=opt)
            runs.append((loss, sums, ops.dice_loss_lowres_bwd(low, y, (ho, wo), sums, up, options=opt)))
        assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------ Dice unchanged
@gpu
def test_dice_is_bit_identical_before_and_after_a_tversky_call():
    """No state is shared between the families: DiceLoss (plain and option kernels, full and low resolution) gives the same
    bits before and after TverskyLoss has run on the same inputs in the same process."""
    B, K, H = 2, 5, 32
    logits, y = uniform(B, K, H, H).to(DEV), make_target((B, H, H), K).to(DEV)
    low = uniform(B, 4, 4, K, seed=3).to(DEV)

    def dice(kw):
        out = []
        for inp in (logits, low):
            leaf = inp.clone().requires_grad_(True)
            loss = gnn.DiceLoss(**kw)(gnn.LowresLogits(leaf, (H, H)) if inp is low else leaf, y)
            (UP * loss).backward()
            out += [loss.detach(), leaf.grad]
        return out

    dice_kws = (dict(), dict(smooth=1.0, log_loss=True, classes=[1, 3]))
    before = [dice(kw) for kw in dice_kws]
    for inp in (logits, low):
        leaf = inp.clone().requires_grad_(True)
        crit = gnn.TverskyLoss(alpha=0.3, beta=0.7, gamma=0.75, smooth=1.0, log_loss=True, classes=[0, 2])
        (UP * crit(gnn.LowresLogits(leaf, (H, H)) if inp is low else leaf, y)).backward()
    after = [dice(kw) for kw in dice_kws]
    for b, a in zip(before, after):
        assert all(torch.equal(x, z) for x, z in zip(b, a))


@gpu
def test_tversky_with_half_weights_is_the_dice_kernels_result():
    """A cross-check between two sets of coefficient code on the same sums: Tversky(alpha = beta = 0.5) against DiceLoss, within
    the loss tolerance both hold against their f64 references."""
    B, K, H = 2, 5, 32
    logits, y = uniform(B, K, H, H).to(DEV), make_target((B, H, H), K).to(DEV)
    a, b = logits.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    lt, ld = gnn.TverskyLoss(alpha=0.5, beta=0.5)(a, y), gnn.DiceLoss()(b, y)
    lt.backward()
    ld.backward()
    assert abs(lt.item() - ld.item()) <= 2 * LOSS_TOL
    assert (a.grad - b.grad).abs().max().item() <= 2 * GRAD_TOL * b.grad.abs().max().item()


# ------------------------------------------------------------------------------------------------ task level
@gpu
def test_dofa_task_with_focal_tversky(monkeypatch):
    """SegmentationDOFA (the tiny config of test_hip_tasks.py) with TverskyLoss(alpha=0.3, beta=0.7, gamma=0.75): the training
    step asks the model for low-resolution logits, gives the f64 restatement's loss on the materialised logits of the same
    model, finite non-zero gradients on both heads' weights, and the same loss and head gradients as the step that materialises
    the logits (FUSE_LOWRES_DICE off, the GDL_LOWRES_DICE=0 semantics).

    Loss bound against the restatement, as in the Dice task test: 2e-6 per low-resolution term (weights 1 and 0.4) plus one f32
    rounding of their sum; between the two GPU paths the sum of the two paths' bounds (1e-6 per term on the materialised one).
    Head gradients: 1e-4 of max|grad|, as for every gradient here."""
    import oracle
    from geo_deep_learning.models.encoders.dofa_v2 import DOFAv2
    from geo_deep_learning.models.segmentation.dofa import DOFASegmentationModel
    from geo_deep_learning.tasks_with_models.segmentation_dofa import SegmentationDOFA
    tiny = dict(patch_size=14, embed_dim=128, depth=4, num_heads=2, out_indices=[0, 1, 2, 3])
    img, nc, b = 112, 5, 4
    kw = dict(alpha=0.3, beta=0.7, gamma=0.75)
    ref = oracle.DOFASegmentationModel("dofa_tiny_test", (img, img), num_classes=nc, _encoder_kwargs=tiny, freeze_layers=["encoder"])
    sd = oracle.procedural_state_dict(ref, 7)
    task = SegmentationDOFA("dofa_base", pretrained=False, image_size=(img, img), num_classes=nc, max_samples=2,
                            loss=gnn.TverskyLoss(mode="multiclass", **kw), freeze_layers=["encoder"],
                            wavelengths=[0.665, 0.549, 0.481])
    task.model = DOFASegmentationModel(DOFAv2(img_size=img, pretrained=False, **tiny), (img, img), num_classes=nc,
                                       pretrained=False, freeze_layers=["encoder"])
    task.configure_model()
    task.model.load_state_dict(sd)
    task = task.to(DEV)

    class _Trainer:
        def __init__(self):
            self.training, self.datamodule, self.estimated_stepping_batches = True, None, 100
            self.accumulate_grad_batches, self.max_epochs = 1, 3

    batch = oracle.synthetic_batch(b, 3, img, nc, 7)
    batch["wavelengths"] = batch["wavelengths"].unsqueeze(0).expand(b, -1).contiguous()
    y = batch["mask"].squeeze(1).long()
    dev = {k: (v.to(DEV) if isinstance(v, torch.Tensor) and k != "wavelengths" else v) for k, v in batch.items()}
    asked = []
    model_forward = task.model.forward

    def spy(*a, **k):
        asked.append(bool(k.get("lowres_logits", False)))
        return model_forward(*a, **k)
    task.model.forward = spy
    task.trainer = _Trainer()
    task.train()
    heads = {n: p for n, p in task.model.named_parameters() if n.startswith(("head.", "aux_head.")) and n.endswith("weight")}
    assert any(n.startswith("head.") for n in heads) and any(n.startswith("aux_head.") for n in heads)

    def step(fused):
        monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", fused)
        asked.clear()
        task.model.zero_grad(set_to_none=True)
        torch.manual_seed(123)      # train mode: the device-RNG draws are repeated by re-seeding
        loss = task.training_step(dev, 0)
        loss.backward()
        assert asked == [fused]
        return loss.detach(), {n: p.grad.clone() for n, p in heads.items()}

    loss, grads = step(True)
    torch.manual_seed(123)
    with torch.no_grad():
        out = task.model(dev["image"], dev["wavelengths"])
    terms = [overlap_ref(t.detach().double().cpu(), y, "tversky", **kw) for t in (out.out, out.aux)]
    want = terms[0][0].item() + 0.4 * terms[1][0].item()
    bound = LOSS_TOL_LOWRES * 1.4 + 2.0 ** -23 * abs(want)
    print(f"train_loss {loss.item():.8f} ref {want:.8f} err {abs(loss.item() - want):.3e} bound {bound:.3e}")
    assert torch.isfinite(loss).item() and abs(loss.item() - want) <= bound
    for n, g in grads.items():
        assert torch.isfinite(g).all().item() and g.abs().max().item() > 0, n
    loss_m, grads_m = step(False)
    bound_m = bound + LOSS_TOL * 1.4 + 2.0 ** -23 * abs(want)
    print(f"materialised {loss_m.item():.8f} diff {abs(loss.item() - loss_m.item()):.3e} bound {bound_m:.3e}")
    assert abs(loss.item() - loss_m.item()) <= bound_m
    for n in grads:
        grad_close(grads[n], grads_m[n], f"task {n}: low-resolution vs materialised step")
