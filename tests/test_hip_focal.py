"""gdlhip.nn.FocalLoss on the GPU: the gdl_focal_* kernels at full resolution, in binary mode and from low-resolution logits
(LowresLogits; tile and gather backward forms), forward and backward with the auxiliary head's upstream factor.

The reference of every number is ``focal_ref`` (tests/test_focal_host.py: smp 0.5.0's arithmetic restated in f64), gradients from
torch autograd, or from ``focal_grad_closed`` where autograd has none (gamma 0.5 at saturated logits); for the low-resolution
family it is applied to ``F.interpolate(low, size, "bilinear")``.  Parity with smp itself is unpinned (not installed).

Shapes, helpers and tolerances are those of tests/test_hip_soft_ce.py: loss within 1e-6 * max(1, |ref|) (2e-6 from low-resolution
logits), gradients within 1e-4 of max|ref|."""

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
    spec = importlib.util.spec_from_file_location(name + "_for_focal", Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_host = _load("test_focal_host")
_sce = _load("test_hip_soft_ce")
focal_ref, focal_grad_closed = _host.focal_ref, _host.focal_grad_closed
rnd, make_target, loss_close, grad_close = _sce.rnd, _sce.make_target, _sce.loss_close, _sce.grad_close
LOSS_TOL, LOSS_TOL_LOWRES, LOWRES_SHAPES = _sce.LOSS_TOL, _sce.LOSS_TOL_LOWRES, _sce.LOWRES_SHAPES

DEV = "cuda"
UP = 0.4          # the upstream factor of the auxiliary head


def check_full(logits, target, mode="multiclass", closed=False, **kw):
    """FocalLoss(mode, **kw) against focal_ref; ``closed``: the gradient against the closed form instead of autograd."""
    x = logits.double().clone().requires_grad_(True)
    ref = focal_ref(x, target, mode=mode, **kw)
    if closed:
        gref = UP * focal_grad_closed(logits.double(), target, mode=mode, **kw)
    else:
        (UP * ref).backward()
        gref = x.grad
    ld = logits.to(DEV).requires_grad_(True)
    loss = gnn.FocalLoss(mode, **kw)(ld, target.to(DEV))
    (UP * loss).backward()
    assert loss.dim() == 0 and torch.isfinite(loss).item() and torch.isfinite(ld.grad).all().item()
    what = f"{mode} {tuple(logits.shape)} {kw}"
    loss_close(loss.item(), ref.item(), LOSS_TOL, what)
    grad_close(ld.grad, gref, what)
    return loss, ld.grad


def check_lowres(shape, form, tgt=None, **kw):
    """FocalLoss("multiclass", **kw) on LowresLogits with the ``form`` backward: against focal_ref on the interpolated logits and
    against the class's own materialised path."""
    B, K, hi, wi, ho, wo = shape
    low = rnd(B, hi, wi, K, seed=3) * 2.0
    if tgt is None:
        tgt = make_target((B, ho, wo), K, kw.get("ignore_index"), seed=4)
    lr = low.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = focal_ref(F.interpolate(lr, size=(ho, wo), mode="bilinear", align_corners=False), tgt, **kw)
    (UP * ref).backward()
    lowd, tgtd = low.to(DEV), tgt.to(DEV)
    crit = gnn.FocalLoss("multiclass", **kw)
    up = torch.tensor(UP, device=DEV)
    la, norm = ops.focal_lowres_fwd(lowd, tgtd, (ho, wo), crit.options)
    ga = ops.focal_lowres_bwd(lowd, tgtd, (ho, wo), norm, up, 1.0, crit.options, form=form)
    b_ = lowd.clone().requires_grad_(True)
    lb = crit(gnn.LowresLogits(b_, (ho, wo)).materialise(), tgtd)
    (UP * lb).backward()
    what = f"lowres {shape} {form} {kw}"
    assert torch.isfinite(la).item() and torch.isfinite(ga).all().item()
    loss_close(la.item(), ref.item(), LOSS_TOL_LOWRES, what)
    loss_close(la.item(), lb.item(), LOSS_TOL, what + " vs the materialised path")
    grad_close(ga.permute(0, 3, 1, 2), lr.grad, what + " vs torch")
    grad_close(ga, b_.grad, what + " vs the materialised path")
    return la, ga


def forms_of(shape):
    B, K, hi, wi, ho, wo = shape
    tiles = gdlhip._lib.load().gdl_focal_lowres_bwd_workspace(B, K, hi, wi, ho, wo) > 0
    assert tiles == (K <= 8)
    return ("tile", "gather") if tiles else ("gather",)


# ------------------------------------------------------------------------------------------------ full resolution
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("ignore", [None, 255, -1])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("alpha", [None, 0.25])
@pytest.mark.parametrize("K", [2, 5, 16, 19])
def test_full_resolution(K, alpha, gamma, ignore, reduction):
    B, H, W = 2, 37, 41
    logits = rnd(B, K, H, W, seed=K) * 2
    y = make_target((B, H, W), K, ignore)
    if ignore is not None:
        assert 0.1 < (y == ignore).float().mean().item() < 0.3
    kw = dict(alpha=alpha, gamma=gamma, ignore_index=ignore, reduction=reduction)
    _, grad = check_full(logits, y, **kw)
    if ignore is not None:
        gi = grad.cpu().permute(0, 2, 3, 1)[y == ignore]
        assert gi.numel() > 0 and (gi == 0).all(), "the gradient of an ignored pixel is exactly 0 in every class"
    # an un-squeezed [B, 1, H, W] mask is the same
    crit = gnn.FocalLoss("multiclass", **kw)
    assert crit(logits.to(DEV), y[:, None].to(DEV)).item() == crit(logits.to(DEV), y.to(DEV)).item()


@pytest.mark.parametrize("gamma", [0.5, 2.0])
@pytest.mark.parametrize("th", [0.5, 0.3])
@pytest.mark.parametrize("K", [2, 5])
def test_reduced_threshold(K, th, gamma):
    """The gradient (for 0.3 the loss too) jumps at pt == th: no element of the data lies within 1e-4 of the switch (the few that
    did were pushed away; tests/test_focal_host.py::test_threshold_nudges_are_a_handful counts them for these seeds)."""
    g = torch.Generator().manual_seed(K)
    x = torch.randn(2, K, 37, 41, generator=g) * 2
    y = torch.randint(0, K, (2, 37, 41), generator=g)
    x, n = _host.nudge_off_threshold(x, y, th)
    assert n <= 8 and _host.threshold_margin(x, y, th) >= 1e-4
    y[0, :4] = 255
    check_full(x, y, alpha=0.25, gamma=gamma, ignore_index=255, reduced_threshold=th)


@pytest.mark.parametrize("K", [5, 19])
def test_out_of_range_target_is_a_valid_all_negative_pixel(K):
    B, H, W = 2, 37, 41
    logits = rnd(B, K, H, W, seed=K) * 2
    y = make_target((B, H, W), K)
    g = torch.Generator().manual_seed(9)
    pick = torch.rand(y.shape, generator=g)
    y[pick < 0.05] = K              # one past the last class
    y[(pick >= 0.05) & (pick < 0.10)] = -3
    y[(pick >= 0.10) & (pick < 0.12)] = 2**33 + 1      # truncates to class 1 as a 32-bit value
    _, grad = check_full(logits, y, alpha=0.25)      # focal_ref compares the target too: no class matches
    gbad = grad.cpu().permute(0, 2, 3, 1)[pick < 0.12]
    assert (gbad > 0).all(), "all-negative pixels: every class is pushed down, none is ignored or taken for class 1"
    none_ignored = gnn.FocalLoss("multiclass", alpha=0.25, ignore_index=K)(logits.to(DEV), y.to(DEV))
    assert none_ignored.item() != gnn.FocalLoss("multiclass", alpha=0.25)(logits.to(DEV), y.to(DEV)).item()


@pytest.mark.parametrize("K", [5, 19])
def test_every_pixel_ignored(K):
    """Loss 0.0, gradient all zero -- full resolution, binary mode and every low-resolution form."""
    B, H = 2, 32
    y = torch.full((B, H, H), 255, dtype=torch.int64, device=DEV)
    ld = (rnd(B, K, H, H) * 2).to(DEV).requires_grad_(True)
    loss = gnn.FocalLoss("multiclass", ignore_index=255)(ld, y)
    (UP * loss).backward()
    assert loss.item() == 0.0 and (ld.grad == 0).all()
    lb = (rnd(B, 1, H, H) * 2).to(DEV).requires_grad_(True)
    loss = gnn.FocalLoss("binary", ignore_index=255)(lb, y)
    (UP * loss).backward()
    assert loss.item() == 0.0 and (lb.grad == 0).all()
    if K <= 16:
        opt, up = ops.FocalOptions(ignore_index=255), torch.tensor(UP, device=DEV)
        low = (rnd(B, 9, 9, K) * 2).to(DEV)
        for form in forms_of((B, K, 9, 9, H, H)):
            loss, norm = ops.focal_lowres_fwd(low, y, (H, H), opt)
            grad = ops.focal_lowres_bwd(low, y, (H, H), norm, up, 1.0, opt, form=form)
            assert loss.item() == 0.0 and norm.item() == 0.0 and (grad == 0).all(), form
        a = low.clone().requires_grad_(True)
        loss = gnn.FocalLoss("multiclass", ignore_index=255)(gnn.LowresLogits(a, (H, H)), y)
        (UP * loss).backward()
        assert loss.item() == 0.0 and (a.grad == 0).all()


@pytest.mark.parametrize("K", [5, 19])
def test_saturated_logits_stay_finite(K):
    """Every logit is +80 or -80.  gamma 2 and 0 against focal_ref; gamma 0.5 against the closed-form gradient (torch's is NaN)."""
    B, H, W = 2, 21, 23
    g = torch.Generator().manual_seed(5)
    logits = (torch.randint(0, 2, (B, K, H, W), generator=g).float() * 2 - 1) * 80.0
    y = make_target((B, H, W), K, 255)
    for reduction in ("mean", "sum"):
        check_full(logits, y, gamma=2.0, alpha=0.25, ignore_index=255, reduction=reduction)
        check_full(logits, y, gamma=0.0, ignore_index=255, reduction=reduction)
        check_full(logits, y, gamma=0.5, ignore_index=255, reduction=reduction, closed=True)


# ------------------------------------------------------------------------------------------------ binary
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_binary(reduction):
    B, H, W = 2, 37, 41
    logits = rnd(B, 1, H, W, seed=1) * 2
    y = make_target((B, 1, H, W), 2, 255)
    assert 0.1 < (y == 255).float().mean().item() < 0.3 and (y == 1).any() and (y == 0).any()
    kw = dict(alpha=0.25, gamma=2.0, ignore_index=255, reduction=reduction)
    loss, grad = check_full(logits, y, mode="binary", **kw)
    assert (grad.cpu()[y == 255] == 0).all()
    # a [B, H, W]-shaped target with equal numel is the same
    flat = gnn.FocalLoss("binary", **kw)(logits.to(DEV), y[:, 0].to(DEV))
    assert torch.equal(flat, loss.detach())
    # any value other than 1 and ignore_index counts as 0
    other = y.clone()
    other[y == 0] = 7
    assert torch.equal(gnn.FocalLoss("binary", **kw)(logits.to(DEV), other.to(DEV)), loss.detach())
    with pytest.raises(ValueError, match="do not match"):
        gnn.FocalLoss("binary")(logits.to(DEV), y[:1].to(DEV))


# ------------------------------------------------------------------------------------------------ low resolution
@pytest.mark.parametrize("kw", [dict(), dict(alpha=0.25, ignore_index=255), dict(gamma=0.5, reduction="sum")],
                         ids=["defaults", "alpha_ignore255", "gamma05_sum"])
@pytest.mark.parametrize("shape", LOWRES_SHAPES)
def test_low_resolution(shape, kw):
    """Every backward form the shape can take (K <= 8: tile and gather; K = 16: gather), each against the f64 reference and the
    materialised path, then against each other; the class itself takes the tile form where there is one."""
    check_forms(shape, kw)


@pytest.mark.parametrize("ignore", [255, None], ids=["ignored", "none_ignored"])
@pytest.mark.parametrize("shape", _sce.SKELETON_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_low_resolution_at_the_tile_edges(shape, ignore):
    """The shapes of tests/test_hip_soft_ce.py::test_low_resolution_at_the_tile_edges."""
    check_forms(shape, dict(alpha=0.25, ignore_index=ignore), _sce.skeleton_target(shape, ignore))


def check_forms(shape, kw, tgt=None):
    forms = forms_of(shape)
    got = {f: check_lowres(shape, f, tgt, **kw) for f in forms}
    base_loss, base_grad = got["gather"]
    for f in forms[:-1]:
        assert torch.equal(got[f][0], base_loss), "the forms share the forward"
        grad_close(got[f][1], base_grad, f"{shape} {f} vs gather backward")
    B, K, hi, wi, ho, wo = shape
    a = (rnd(B, hi, wi, K, seed=3) * 2.0).to(DEV).requires_grad_(True)
    y = (make_target((B, ho, wo), K, kw.get("ignore_index"), seed=4) if tgt is None else tgt).to(DEV)
    loss = gnn.FocalLoss("multiclass", **kw)(gnn.LowresLogits(a, (ho, wo)), y[:, None])
    (UP * loss).backward()
    assert torch.equal(loss.detach(), base_loss) and torch.equal(a.grad, got[forms[0]][1])


def test_shapes_outside_the_kernel_limits_materialise():
    """A downsample is not a shape gdl_focal_lowres_* take: the class resizes first and runs the full-resolution kernels."""
    low = (rnd(2, 12, 12, 5) * 2).to(DEV).requires_grad_(True)
    y = make_target((2, 8, 8), 5).to(DEV)
    assert not ops.focal_lowres_ok(low, (8, 8))
    lr = low.detach().double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    ref = focal_ref(F.interpolate(lr, size=(8, 8), mode="bilinear", align_corners=False), y.cpu(), alpha=0.25)
    ref.backward()
    loss = gnn.FocalLoss("multiclass", alpha=0.25)(gnn.LowresLogits(low, (8, 8)), y)
    loss.backward()
    loss_close(loss.item(), ref.item(), LOSS_TOL_LOWRES, "materialised downsample")
    grad_close(low.grad.permute(0, 3, 1, 2), lr.grad, "materialised downsample")


# ------------------------------------------------------------------------------------------------ determinism, accumulation, errors
def test_two_calls_give_the_same_bits():
    up = torch.tensor(UP, device=DEV)
    opt = ops.FocalOptions(2.0, 0.25, 255, True, None)
    for K in (5, 19):
        logits, y = (rnd(4, K, 67, 129) * 2).to(DEV), make_target((4, 67, 129), K, 255).to(DEV)
        runs = []
        for _ in range(2):
            loss, norm = ops.focal_fwd(logits, y, opt)
            runs.append((loss, norm, ops.focal_bwd(logits, y, norm, up, 1.0, opt)))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), K
    for shape in LOWRES_SHAPES:
        B, K, hi, wi, ho, wo = shape
        low, y = (rnd(B, hi, wi, K, seed=3) * 2).to(DEV), make_target((B, ho, wo), K, 255, seed=4).to(DEV)
        for form in forms_of(shape):
            runs = []
            for _ in range(2):
                loss, norm = ops.focal_lowres_fwd(low, y, (ho, wo), opt)
                runs.append((loss, norm, ops.focal_lowres_bwd(low, y, (ho, wo), norm, up, 1.0, opt, form=form)))
            assert all(torch.equal(a, b) for a, b in zip(*runs)), (shape, form)


def test_backward_accumulates_into_an_existing_gradient():
    up = torch.tensor(UP, device=DEV)
    logits, y = (rnd(2, 5, 20, 20) * 2).to(DEV), make_target((2, 20, 20), 5).to(DEV)
    _, norm = ops.focal_fwd(logits, y)
    g = ops.focal_bwd(logits, y, norm, up, 0.5)
    acc = torch.ones_like(logits)
    ops.focal_bwd(logits, y, norm, up, 0.5, out=acc, accumulate=True)
    assert torch.equal(acc, 1.0 + g)
    lb, yb = logits[:, :1].contiguous(), make_target((2, 1, 20, 20), 2).to(DEV)
    _, norm = ops.focal_binary_fwd(lb, yb)
    g = ops.focal_binary_bwd(lb, yb, norm, up, 0.5)
    acc = torch.ones_like(lb)
    ops.focal_binary_bwd(lb, yb, norm, up, 0.5, out=acc, accumulate=True)
    assert torch.equal(acc, 1.0 + g)


def test_c_entry_points_return_error_codes():
    logits, y = torch.zeros(1, 3, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="gamma"):
        ops.focal_fwd(logits, y, ops.FocalOptions(gamma=-1.0))
    with pytest.raises(ValueError, match="gamma"):
        ops.focal_fwd(logits, y, ops.FocalOptions(gamma=float("nan")))
    with pytest.raises(ValueError, match="alpha"):
        ops.focal_binary_fwd(logits[:, :1].contiguous(), y, ops.FocalOptions(alpha=1.5))
    with pytest.raises(ValueError, match="reduced_threshold"):
        ops.focal_fwd(logits, y, ops.FocalOptions(reduced_threshold=0.0))
    low, norm = torch.zeros(1, 2, 2, 17, device=DEV), torch.ones(1, device=DEV)
    with pytest.raises(ValueError, match="K=17"):
        ops.focal_lowres_fwd(low, y, (4, 4))
    with pytest.raises(ValueError, match="K=17"):
        ops.focal_lowres_bwd(low, y, (4, 4), norm, None)
    with pytest.raises(ValueError, match="tile form"):      # K = 16 has no tile form
        ops.focal_lowres_bwd(low[..., :16].contiguous(), y, (4, 4), norm, None, form="tile")


# ------------------------------------------------------------------------------------------------ task level
def test_dofa_training_step_from_low_resolution_logits_equals_the_materialised_step(monkeypatch):
    """One SegmentationDOFA training step on the tiny configuration of the task tests with FocalLoss("multiclass", alpha=0.25):
    the step asks the model for LowresLogits, its loss equals the step with FUSE_LOWRES_DICE off (full-resolution logits written
    and read) within LOSS_TOL_LOWRES, and every trainable parameter has a finite gradient."""
    task = _sce._dofa_task(gnn.FocalLoss("multiclass", alpha=0.25))
    dev = _sce._dofa_batch(7)
    asked = []
    model_forward = task.model.forward

    def spy(*a, **kw):
        asked.append(bool(kw.get("lowres_logits", False)))
        return model_forward(*a, **kw)
    task.model.forward = spy
    task.train()
    losses = {}
    for fuse in (True, False):
        monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", fuse)
        task.zero_grad(set_to_none=True)
        torch.manual_seed(123)
        loss = task.training_step(dev, 0)
        loss.backward()
        losses[fuse] = loss.item()
        trainable = [(n, p) for n, p in task.model.named_parameters() if p.requires_grad]
        assert len(trainable) > 30
        for n, p in trainable:
            assert p.grad is not None and torch.isfinite(p.grad).all().item(), n
        assert any(p.grad.abs().max().item() > 0 for _, p in trainable)
    assert asked == [True, False]
    loss_close(losses[True], losses[False], LOSS_TOL_LOWRES, "dofa step: lowres vs materialised")


def test_graphed_train_step_reproduces_the_eager_losses_bit_for_bit():
    """GraphedTrainStep (hipGraph capture of forward + FocalLoss from low-resolution logits + backward + Adam) on the tiny DOFA
    task: one capture and two replays against the same steps run eagerly, bit for bit.  In a process of its own
    (tests/_loss_graph_worker.py, scenario "focal"), one capture scenario per process as tests/_graph_interleave_worker.py explains."""
    worker = Path(__file__).with_name("_loss_graph_worker.py")
    run = subprocess.run([sys.executable, str(worker), "focal"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    print(res)
    assert len(res["eager"]) == 2 and res["eager"] == res["graphed"], res
