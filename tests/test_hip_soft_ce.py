"""gdlhip.nn.SoftCrossEntropyLoss on the GPU: the gdl_soft_ce_* kernels at full resolution and from low-resolution logits
(LowresLogits; fused, tile-recompute and gather backward forms), forward and backward with the auxiliary head's upstream factor.

The reference of every number is ``soft_ce_ref`` (tests/test_soft_ce_host.py: smp 0.5.0's formula restated in f64, tied there
to ``F.cross_entropy(label_smoothing=e, reduction="sum") / N``), gradients from torch autograd; for the low-resolution family
it is applied to ``F.interpolate(low, size, "bilinear")``.  Parity with smp itself is unpinned (not installed).

Tolerances are those of test_hip_dice_options.py, taken relative to max(1, |ref|) because cross-entropy is unbounded: loss
within 1e-6 (2e-6 from low-resolution logits), gradients within 1e-4 of max|ref|."""

import importlib.util
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402

_spec = importlib.util.spec_from_file_location("soft_ce_host_reference", Path(__file__).with_name("test_soft_ce_host.py"))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)
soft_ce_ref = _host.soft_ce_ref      # the f64 restatement, tied to F.cross_entropy there

DEV = "cuda"
UP = 0.4          # the upstream factor of the auxiliary head
LOSS_TOL, LOSS_TOL_LOWRES, GRAD_TOL = 1e-6, 2e-6, 1e-4


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)))


def make_target(shape, k, ignore=None, frac=0.2, seed=1):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, k, shape, generator=g)
    if ignore is not None:
        t[torch.rand(shape, generator=g) < frac] = ignore
    return t


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


def check_full(logits, target, ref_target=None, **kw):
    """SoftCrossEntropyLoss(**kw) on full-resolution logits against soft_ce_ref (on ``ref_target`` when given)."""
    x = logits.double().clone().requires_grad_(True)
    ref = soft_ce_ref(x, target if ref_target is None else ref_target, kw.get("smooth_factor"), kw.get("ignore_index", -100),
                      kw.get("reduction", "mean"))
    (UP * ref).backward()
    ld = logits.to(DEV).requires_grad_(True)
    loss = gnn.SoftCrossEntropyLoss(**kw)(ld, target.to(DEV))
    (UP * loss).backward()
    assert loss.dim() == 0 and torch.isfinite(loss).item() and torch.isfinite(ld.grad).all().item()
    loss_close(loss.item(), ref.item(), LOSS_TOL, f"full {tuple(logits.shape)} {kw}")
    grad_close(ld.grad, x.grad, f"full {tuple(logits.shape)} {kw}")
    return loss, ld.grad


class Form:
    """Selects the low-resolution backward form for the duration of a ``with`` block: "fused", "tile" or "gather"."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.lib = gdlhip._lib.load()
        self.keep = gnn.SOFT_CE_LOWRES_FUSED
        gnn.SOFT_CE_LOWRES_FUSED = self.form == "fused"
        self.lib.gdl_debug_set_soft_ce_lowres_tiled(0 if self.form == "gather" else 1)

    def __exit__(self, *exc):
        gnn.SOFT_CE_LOWRES_FUSED = self.keep
        self.lib.gdl_debug_set_soft_ce_lowres_tiled(1)


def check_lowres(shape, form, tgt=None, **kw):
    """SoftCrossEntropyLoss(**kw) on LowresLogits through ``form``: against soft_ce_ref on the interpolated logits and against
    the class's own materialised path."""
    B, K, hi, wi, ho, wo = shape
    low = rnd(B, hi, wi, K, seed=3) * 2.0
    if tgt is None:
        tgt = make_target((B, ho, wo), K, kw.get("ignore_index", -100), seed=4)
    lr = low.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = soft_ce_ref(F.interpolate(lr, size=(ho, wo), mode="bilinear", align_corners=False), tgt, kw.get("smooth_factor"),
                      kw.get("ignore_index", -100), kw.get("reduction", "mean"))
    (UP * ref).backward()
    lowd, tgtd = low.to(DEV), tgt.to(DEV)
    crit = gnn.SoftCrossEntropyLoss(**kw)
    a = lowd.clone().requires_grad_(True)
    b_ = lowd.clone().requires_grad_(True)
    with Form(form):
        la = crit(gnn.LowresLogits(a, (ho, wo)), tgtd)
        (UP * la).backward()
    lb = crit(gnn.LowresLogits(b_, (ho, wo)).materialise(), tgtd)
    (UP * lb).backward()
    what = f"lowres {shape} {form} {kw}"
    assert torch.isfinite(la).item() and torch.isfinite(a.grad).all().item()
    loss_close(la.item(), ref.item(), LOSS_TOL_LOWRES, what)
    loss_close(la.item(), lb.item(), LOSS_TOL, what + " vs the materialised path")
    grad_close(a.grad.permute(0, 3, 1, 2), lr.grad, what + " vs torch")
    grad_close(a.grad, b_.grad, what + " vs the materialised path")
    return la, a.grad


# ------------------------------------------------------------------------------------------------ full resolution
@pytest.mark.parametrize("ignore", [None, -100, 255])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("K", [2, 5, 16, 19])
def test_full_resolution(K, eps, reduction, ignore):
    B, H, W = 2, 37, 41
    logits = rnd(B, K, H, W, seed=K) * 2
    y = make_target((B, H, W), K, ignore)
    if ignore is not None:
        assert 0.1 < (y == ignore).float().mean().item() < 0.3
    _, grad = check_full(logits, y, reduction=reduction, smooth_factor=eps, ignore_index=ignore)
    if ignore is not None:
        gi = grad.cpu().permute(0, 2, 3, 1)[y == ignore]
        assert gi.numel() > 0 and (gi == 0).all(), "the gradient of an ignored pixel is exactly 0 in every class"
    # an un-squeezed [B, 1, H, W] mask is the same
    crit = gnn.SoftCrossEntropyLoss(reduction=reduction, smooth_factor=eps, ignore_index=ignore)
    assert crit(logits.to(DEV), y[:, None].to(DEV)).item() == crit(logits.to(DEV), y.to(DEV)).item()


@pytest.mark.parametrize("K", [5, 19])
def test_out_of_range_target_is_treated_as_ignored(K):
    B, H, W = 2, 37, 41
    logits = rnd(B, K, H, W, seed=K) * 2
    y = make_target((B, H, W), K, -100)
    bad = y.clone()
    g = torch.Generator().manual_seed(9)
    pick = torch.rand(y.shape, generator=g)
    bad[pick < 0.05] = K              # one past the last class
    bad[(pick >= 0.05) & (pick < 0.10)] = -3
    bad[(pick >= 0.10) & (pick < 0.12)] = 2**33 + 1      # truncates to class 1 as a 32-bit value
    want = y.clone()
    want[pick < 0.12] = -100
    _, grad = check_full(logits, bad, ref_target=want, smooth_factor=0.1)
    assert (grad.cpu().permute(0, 2, 3, 1)[pick < 0.12] == 0).all()


@pytest.mark.parametrize("K", [5, 19])
def test_every_pixel_ignored(K):
    """Loss 0, gradient all zero, everything finite -- full resolution and every low-resolution form."""
    B, H = 2, 32
    y = torch.full((B, H, H), -100, dtype=torch.int64, device=DEV)
    ld = (rnd(B, K, H, H) * 2).to(DEV).requires_grad_(True)
    loss = gnn.SoftCrossEntropyLoss(smooth_factor=0.1)(ld, y)
    (UP * loss).backward()
    assert loss.item() == 0.0 and (ld.grad == 0).all()
    if K <= 16:
        for form in ("fused", "tile", "gather"):
            low = (rnd(B, 9, 9, K) * 2).to(DEV).requires_grad_(True)
            with Form(form):
                loss = gnn.SoftCrossEntropyLoss(smooth_factor=0.1)(gnn.LowresLogits(low, (H, H)), y)
                (UP * loss).backward()
            assert loss.item() == 0.0 and (low.grad == 0).all(), form


@pytest.mark.parametrize("K", [5, 19])
def test_large_logits_stay_finite(K):
    B, H, W = 2, 21, 23
    g = torch.Generator().manual_seed(5)
    logits = (torch.randint(0, 2, (B, K, H, W), generator=g).float() * 2 - 1) * 80.0      # every logit is +80 or -80
    y = make_target((B, H, W), K, 255)
    for reduction in ("mean", "sum"):
        check_full(logits, y, reduction=reduction, smooth_factor=0.1, ignore_index=255)


def test_without_smoothing_and_ignored_pixels_it_is_torch_cross_entropy():
    B, K, H, W = 2, 5, 37, 41
    logits, y = rnd(B, K, H, W) * 2, make_target((B, H, W), K)
    x = logits.double().requires_grad_(True)
    ref = F.cross_entropy(x, y, reduction="mean")
    (UP * ref).backward()
    ld = logits.to(DEV).requires_grad_(True)
    loss = gnn.SoftCrossEntropyLoss()(ld, y.to(DEV))
    (UP * loss).backward()
    loss_close(loss.item(), ref.item(), LOSS_TOL, "vs F.cross_entropy")
    grad_close(ld.grad, x.grad, "vs F.cross_entropy")
    low = rnd(B, 9, 9, K, seed=3) * 2
    lr = low.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = F.cross_entropy(F.interpolate(lr, size=(H, W), mode="bilinear", align_corners=False), y, reduction="mean")
    (UP * ref).backward()
    a = low.to(DEV).requires_grad_(True)
    loss = gnn.SoftCrossEntropyLoss()(gnn.LowresLogits(a, (H, W)), y.to(DEV))
    (UP * loss).backward()
    loss_close(loss.item(), ref.item(), LOSS_TOL_LOWRES, "lowres vs F.cross_entropy")
    grad_close(a.grad.permute(0, 3, 1, 2), lr.grad, "lowres vs F.cross_entropy")


# ------------------------------------------------------------------------------------------------ low resolution
# the shape families of test_hip_dice_options.py::check_lowres (integer and non-integer factors, K <= 8 and K > 8) plus both DOFA
# heads: 144 -> 512 (factor 3.56) and 18 -> 512 (the second shape)
LOWRES_SHAPES = [(2, 5, 36, 36, 128, 128), (2, 5, 18, 18, 512, 512), (3, 16, 6, 10, 50, 41), (2, 5, 9, 9, 32, 32),
                 (2, 5, 144, 144, 512, 512)]


# The tile-edge and window cases of the kernel skeletons every low-resolution loss shares (csrc/lowres_tile.h; tiles are 32 x 64):
# one partial tile; remainder tiles of one pixel in each direction at a non-integer ratio; the largest factor; 1:1 in one direction
# only; 1:1 in both.  K = 8 is the tile limit, K = 9 and 16 take the gather kernel.
SKELETON_SIZES = [(4, 4, 8, 8), (5, 7, 33, 65), (1, 1, 64, 64), (8, 8, 8, 16), (8, 8, 8, 8)]
SKELETON_SHAPES = [(2, K, *size) for size in SKELETON_SIZES for K in (5, 8, 9, 16)]


def skeleton_target(shape, ignore):
    """With ``ignore``: a quarter of the pixels at random plus the whole first 32 x 64 tile of image 0."""
    B, K, hi, wi, ho, wo = shape
    tgt = make_target((B, ho, wo), K, ignore, frac=0.25, seed=4)
    if ignore is not None:
        tgt[0, :32, :64] = ignore
    return tgt


def check_forms(shape, kw, tgt=None):
    B, K, hi, wi, ho, wo = shape
    lib = gdlhip._lib.load()
    tiles = lib.gdl_soft_ce_lowres_fused_state(B, K, hi, wi, ho, wo) > 0
    assert tiles == (K <= 8)
    assert (lib.gdl_soft_ce_lowres_bwd_workspace(B, K, hi, wi, ho, wo) > 0) == tiles
    forms = ("fused", "tile", "gather") if tiles else ("gather",)
    got = {f: check_lowres(shape, f, tgt, **kw) for f in forms}
    base_loss, base_grad = got["gather"]
    for f in forms[:-1]:
        loss_close(got[f][0].item(), base_loss.item(), LOSS_TOL, f"{shape} {f} vs gather")
        grad_close(got[f][1], base_grad, f"{shape} {f} vs gather backward")
    if tiles:
        assert torch.equal(got["tile"][0], got["gather"][0]), "the two recompute forms share the forward"


@pytest.mark.parametrize("kw", [dict(), dict(smooth_factor=0.1, ignore_index=255), dict(smooth_factor=0.1, reduction="sum", ignore_index=None)],
                         ids=["defaults", "smooth_ignore255", "smooth_sum_noignore"])
@pytest.mark.parametrize("shape", LOWRES_SHAPES)
def test_low_resolution(shape, kw):
    """Every backward form the shape can take, each against the f64 reference and the materialised path, then against each
    other.  K <= 8 takes the fused form by default and the tile kernel in the recompute form; K > 8 the gather kernel."""
    check_forms(shape, kw)


@pytest.mark.parametrize("ignore", [255, None], ids=["ignored", "none_ignored"])
@pytest.mark.parametrize("shape", SKELETON_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_low_resolution_at_the_tile_edges(shape, ignore):
    check_forms(shape, dict(smooth_factor=0.1, ignore_index=ignore), skeleton_target(shape, ignore))


def test_low_resolution_out_of_range_target_and_unsqueezed_mask():
    B, K, hi, ho = 2, 5, 9, 32
    low = (rnd(B, hi, hi, K, seed=3) * 2).to(DEV)
    y = make_target((B, ho, ho), K, -100, seed=4)
    bad = y.clone()
    bad[:, :3] = K + 2
    want = y.clone()
    want[:, :3] = -100
    crit = gnn.SoftCrossEntropyLoss(smooth_factor=0.1)
    for form in ("fused", "tile", "gather"):
        a, b_ = low.clone().requires_grad_(True), low.clone().requires_grad_(True)
        with Form(form):
            la = crit(gnn.LowresLogits(a, (ho, ho)), bad.to(DEV))
            lb = crit(gnn.LowresLogits(b_, (ho, ho)), want[:, None].to(DEV))
            (la + lb).backward()
        assert torch.equal(la, lb) and torch.equal(a.grad, b_.grad), form


def test_shapes_outside_the_kernel_limits_materialise():
    """A downsample is not a shape gdl_soft_ce_lowres_* take: the class resizes first and runs the full-resolution kernels."""
    low = (rnd(2, 12, 12, 5) * 2).to(DEV).requires_grad_(True)
    y = make_target((2, 8, 8), 5).to(DEV)
    assert not ops.soft_ce_lowres_ok(low, (8, 8))
    lr = low.detach().double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    ref = soft_ce_ref(F.interpolate(lr, size=(8, 8), mode="bilinear", align_corners=False), y.cpu(), 0.1)
    loss = gnn.SoftCrossEntropyLoss(smooth_factor=0.1)(gnn.LowresLogits(low, (8, 8)), y)
    loss.backward()
    loss_close(loss.item(), ref.item(), LOSS_TOL_LOWRES, "materialised downsample")


# ------------------------------------------------------------------------------------------------ determinism
def test_two_calls_give_the_same_bits():
    up = torch.tensor(UP, device=DEV)
    opt = ops.SoftCEOptions(0.1, 255, True)
    for K in (5, 19):
        logits, y = (rnd(4, K, 67, 129) * 2).to(DEV), make_target((4, 67, 129), K, 255).to(DEV)
        runs = [(ops.soft_ce_fwd(logits, y, opt), ops.soft_ce_bwd(logits, y, up, 1.0, opt)) for _ in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(*runs)), K
    for shape in LOWRES_SHAPES:
        B, K, hi, wi, ho, wo = shape
        low, y = (rnd(B, hi, wi, K, seed=3) * 2).to(DEV), make_target((B, ho, wo), K, 255, seed=4).to(DEV)
        for form in ("fused", "tile", "gather") if K <= 8 else ("gather",):
            runs = []
            with Form(form):
                for _ in range(2):
                    loss, state = ops.soft_ce_lowres_fwd(low, y, (ho, wo), opt, fused=form == "fused")
                    assert (state is not None) == (form == "fused")
                    runs.append((loss, ops.soft_ce_lowres_bwd(low, y, (ho, wo), up, 1.0, opt, state=state)))
            assert all(torch.equal(a, b) for a, b in zip(*runs)), (shape, form)


def test_backward_accumulates_into_an_existing_gradient():
    logits, y = (rnd(2, 5, 20, 20) * 2).to(DEV), make_target((2, 20, 20), 5).to(DEV)
    up = torch.tensor(UP, device=DEV)
    g = ops.soft_ce_bwd(logits, y, up, 0.5)
    acc = torch.ones_like(logits)
    ops.soft_ce_bwd(logits, y, up, 0.5, out=acc, accumulate=True)
    assert torch.equal(acc, 1.0 + g)


def test_c_entry_points_return_error_codes():
    logits, y = torch.zeros(1, 3, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="smooth_factor"):
        ops.soft_ce_fwd(logits, y, ops.SoftCEOptions(1.5, None, True))
    low = torch.zeros(1, 2, 2, 17, device=DEV)
    with pytest.raises((ValueError, NotImplementedError, RuntimeError)):
        ops.soft_ce_lowres_fwd(low, y, (4, 4))


# ------------------------------------------------------------------------------------------------ task level
def _param_grads_close(model, ref, tol=3e-2, floor=2e-6):
    """The per-parameter bound of test_hip_unetpp.py::test_unetpp_train_step_matches_oracle / test_hip_tasks.py::_grads_close."""
    refp = dict(ref.named_parameters())
    bad, n = [], 0
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        err, rn = (p.grad.float().cpu() - refp[name].grad).norm().item(), refp[name].grad.norm().item()
        if err > tol * rn + floor:
            bad.append((name, err, rn))
        n += 1
    assert not bad, bad[:8]
    return n


def test_quickstart_shaped_unetplus_step_matches_the_oracle():
    """The quick-start notebook's configuration (UNet++ / ResNet34, 3 bands, 2 classes, SoftCrossEntropyLoss(smooth_factor=0.1))
    on small synthetic tiles: one training step against oracle/unetpp.py in f32 with the reference loss, to the bounds
    test_hip_unetpp.py::test_unetpp_train_step_matches_oracle uses (loss 1e-5, per-parameter gradient 3e-2 of its norm + 2e-6)."""
    from geo_deep_learning.tasks_with_models.segmentation_unetplus import SegmentationUnetPlus
    from oracle import procedural_state_dict, synthetic_batch
    from oracle.unetpp import UnetPlusPlus as OracleUnetPlusPlus
    seed, b = 9, 2
    ora = OracleUnetPlusPlus("resnet34", 3, 2)
    sd = procedural_state_dict(ora, seed)
    ora.load_state_dict(sd)
    task = SegmentationUnetPlus(encoder="resnet34", image_size=(128, 128), in_channels=3, num_classes=2, max_samples=2,
                                loss=gnn.SoftCrossEntropyLoss(smooth_factor=0.1))
    task.configure_model()
    task.model.load_state_dict(sd)
    task = task.to(DEV)
    batch = synthetic_batch(b, 3, 128, 2, seed)
    dev = {k: (v.to(DEV) if isinstance(v, torch.Tensor) and k != "wavelengths" else v) for k, v in batch.items()}

    class _Trainer:
        training, datamodule, estimated_stepping_batches, accumulate_grad_batches, max_epochs = True, None, 100, 1, 3
    task.trainer = _Trainer()
    task.train(); ora.train()
    loss = task.training_step(dev, 0)
    loss.backward()
    lo = soft_ce_ref(ora(batch["image"]), batch["mask"].squeeze(1).long(), 0.1)
    lo.backward()
    print(f"unet++ quick-start step: loss {loss.item():.8f} oracle {lo.item():.8f}")
    assert abs(loss.item() - lo.item()) < 1e-5
    assert _param_grads_close(task.model, ora) > 100


def _dofa_task(loss, capturable=None):
    import oracle
    from geo_deep_learning.models.encoders.dofa_v2 import DOFAv2
    from geo_deep_learning.models.segmentation.dofa import DOFASegmentationModel
    from geo_deep_learning.tasks_with_models.segmentation_dofa import SegmentationDOFA
    tiny = dict(patch_size=14, embed_dim=128, depth=4, num_heads=2, out_indices=[0, 1, 2, 3])
    img, nc = 112, 5
    ref = oracle.DOFASegmentationModel("dofa_tiny_test", (img, img), num_classes=nc, _encoder_kwargs=tiny, freeze_layers=["encoder"])
    sd = oracle.procedural_state_dict(ref, 7)
    task = SegmentationDOFA("dofa_base", pretrained=False, image_size=(img, img), num_classes=nc, max_samples=2, loss=loss,
                            freeze_layers=["encoder"], wavelengths=[0.665, 0.549, 0.481])
    task.model = DOFASegmentationModel(DOFAv2(img_size=img, pretrained=False, **tiny), (img, img), num_classes=nc,
                                       pretrained=False, freeze_layers=["encoder"])
    task.configure_model()
    task.model.load_state_dict(sd)
    task = task.to(DEV)

    class _Trainer:
        training, datamodule, estimated_stepping_batches, accumulate_grad_batches, max_epochs = True, None, 100, 1, 3
    task.trainer = _Trainer()
    return task


def _dofa_batch(seed, b=4):
    import oracle
    batch = oracle.synthetic_batch(b, 3, 112, 5, seed)
    batch["wavelengths"] = batch["wavelengths"].unsqueeze(0).expand(b, -1).contiguous()
    batch["mask"] = batch["mask"].long()
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) and k != "wavelengths" else v) for k, v in batch.items()}


def test_dofa_training_step_from_low_resolution_logits_equals_the_materialised_step(monkeypatch):
    """One SegmentationDOFA training step with SoftCrossEntropyLoss(smooth_factor=0.1, ignore_index=255): the step that hands the
    loss the heads' own maps equals the step with GDL_LOWRES_DICE=0 (full-resolution logits written and read), to the bounds
    test_hip_tasks.py holds a DOFA training step to (loss 1e-5; per-parameter gradient 3e-2 of its norm + 2e-6), and the loss
    equals the f64 reference on the materialised logits."""
    task = _dofa_task(gnn.SoftCrossEntropyLoss(smooth_factor=0.1, ignore_index=255))
    dev = _dofa_batch(7)
    g = torch.Generator().manual_seed(5)
    dev["mask"][(torch.rand(dev["mask"].shape, generator=g) < 0.2).to(DEV)] = 255
    asked = []
    model_forward = task.model.forward

    def spy(*a, **kw):
        asked.append(bool(kw.get("lowres_logits", False)))
        return model_forward(*a, **kw)
    task.model.forward = spy
    task.train()
    steps = {}
    for fuse in (True, False):
        monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", fuse)
        task.zero_grad(set_to_none=True)
        torch.manual_seed(123)
        loss = task.training_step(dev, 0)
        loss.backward()
        steps[fuse] = (loss.item(), {n: p.grad.clone() for n, p in task.model.named_parameters() if p.grad is not None})
    assert asked == [True, False]
    torch.manual_seed(123)
    with torch.no_grad():
        o = task.model(dev["image"], dev["wavelengths"])
    y = dev["mask"].squeeze(1).cpu()
    want = sum(w * soft_ce_ref(t.double().cpu(), y, 0.1, 255).item() for w, t in ((1.0, o.out), (0.4, o.aux)))
    print(f"dofa step: lowres {steps[True][0]:.8f} materialised {steps[False][0]:.8f} f64 reference {want:.8f}")
    assert abs(steps[True][0] - steps[False][0]) < 1e-5 and abs(steps[True][0] - want) < 1e-5
    assert len(steps[True][1]) > 30 and steps[True][1].keys() == steps[False][1].keys()
    for n, ga in steps[True][1].items():
        gb = steps[False][1][n]
        err, rn = (ga - gb).norm().item(), gb.norm().item()
        assert err <= 3e-2 * rn + 2e-6, (n, err, rn)
    assert any(g_.abs().max().item() > 0 for g_ in steps[True][1].values())


def test_graphed_train_step_reproduces_the_eager_losses_bit_for_bit():
    """GraphedTrainStep (hipGraph capture of forward + SoftCrossEntropyLoss from low-resolution logits + backward + Adam) against
    the same steps run eagerly: bit-identical losses over three replays.  Stochastic layers are off and the optimizer runs
    without gradient clipping, because the gradient-norm reduction adds with float atomics (its bits differ from run to run);
    everything else in the step, the new kernels included, has a fixed summation order."""
    from gdlhip.graphs import GraphedTrainStep

    def make(capturable):
        task = _dofa_task(gnn.SoftCrossEntropyLoss(smooth_factor=0.1))
        for blk in task.model.encoder.blocks:
            blk.drop_prob = 0.0
        task.model.aux_head.dropout_ratio = 0.0
        params = [p for p in task.parameters() if p.requires_grad]
        return task, gnn.FusedAdam(params, lr=1e-3, capturable=capturable)

    batches = [_dofa_batch(30 + i, b=2) for i in range(4)]
    te, oe = make(False)
    tg, og = make(True)
    graphed = GraphedTrainStep(tg, og, batches[0], autocast_dtype=None, warmup=2)
    te.train()
    for _ in range(2):      # the two warm-up steps were real optimizer steps on batches[0]
        oe.zero_grad(set_to_none=True)
        te.training_step(batches[0], 0).backward()
        oe.step()
    for i, b in enumerate(batches[1:]):
        oe.zero_grad(set_to_none=True)
        le = te.training_step(b, 0)
        le.backward()
        oe.step()
        lg = graphed(b)
        print(f"replay {i}: eager {le.item():.9f} graphed {lg.item():.9f}")
        assert torch.equal(le.detach(), lg.detach()), (i, le.item(), lg.item())
