"""gdlhip.nn.CrossEntropyLoss on the GPU: the gdl_cross_entropy_* kernels at full resolution and from low-resolution logits
(LowresLogits; tile and gather backward forms), forward and backward with the auxiliary head's upstream factor.

The reference of every number is ``F.cross_entropy`` in f64 on the CPU and its autograd gradient; for the low-resolution family
it is applied to ``F.interpolate(low, size, "bilinear", align_corners=False)``.  Where torch cannot be the reference -- an
out-of-range target, a zero divisor -- it is ``cross_entropy_ref`` (tests/test_cross_entropy_host.py: the same formula in f64,
tied to ``F.cross_entropy`` there).

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
    spec = importlib.util.spec_from_file_location(name + "_for_cross_entropy", Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_host = _load("test_cross_entropy_host")
_sce = _load("test_hip_soft_ce")
cross_entropy_ref, class_weights = _host.cross_entropy_ref, _host.class_weights
rnd, make_target, loss_close, grad_close = _sce.rnd, _sce.make_target, _sce.loss_close, _sce.grad_close
LOSS_TOL, LOSS_TOL_LOWRES, LOWRES_SHAPES, SKELETON_SHAPES = _sce.LOSS_TOL, _sce.LOSS_TOL_LOWRES, _sce.LOWRES_SHAPES, _sce.SKELETON_SHAPES

DEV = "cuda"
UP = 0.4          # the upstream factor of the auxiliary head
NO_IGNORE = -(2**40)      # F.cross_entropy's ignore_index is an int: a value no target holds stands for None


def torch_ref(x, y, weight=None, ignore_index=-100, reduction="mean", label_smoothing=0.0):
    return F.cross_entropy(x, y, weight=None if weight is None else weight.double(),
                           ignore_index=NO_IGNORE if ignore_index is None else ignore_index, reduction=reduction,
                           label_smoothing=label_smoothing)


def check_full(logits, target, ref=torch_ref, ref_target=None, **kw):
    """CrossEntropyLoss(**kw) on full-resolution logits against ``ref`` in f64 (on ``ref_target`` when given)."""
    x = logits.double().clone().requires_grad_(True)
    want = ref(x, target if ref_target is None else ref_target, **kw)
    (UP * want).backward()
    ld = logits.to(DEV).requires_grad_(True)
    loss = gnn.CrossEntropyLoss(**kw).to(DEV)(ld, target.to(DEV))
    (UP * loss).backward()
    assert loss.dim() == 0 and torch.isfinite(loss).item() and torch.isfinite(ld.grad).all().item()
    what = f"full {tuple(logits.shape)} {kw}"
    loss_close(loss.item(), want.item(), LOSS_TOL, what)
    grad_close(ld.grad, x.grad, what)
    return loss, ld.grad


def check_lowres(shape, form, tgt=None, **kw):
    """CrossEntropyLoss(**kw) from low-resolution logits with the ``form`` backward: against F.cross_entropy on the interpolated
    logits and against the class's own materialised path."""
    B, K, hi, wi, ho, wo = shape
    low = rnd(B, hi, wi, K, seed=3) * 2.0
    if tgt is None:
        tgt = make_target((B, ho, wo), K, kw.get("ignore_index", -100), seed=4)
    lr = low.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = torch_ref(F.interpolate(lr, size=(ho, wo), mode="bilinear", align_corners=False), tgt, **kw)
    (UP * ref).backward()
    lowd, tgtd = low.to(DEV), tgt.to(DEV)
    crit = gnn.CrossEntropyLoss(**kw).to(DEV)
    opt, up = crit._options(K), torch.tensor(UP, device=DEV)
    la, norm = ops.cross_entropy_lowres_fwd(lowd, tgtd, (ho, wo), opt)
    ga = ops.cross_entropy_lowres_bwd(lowd, tgtd, (ho, wo), norm, up, 1.0, opt, form=form)
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
    tiles = gdlhip._lib.load().gdl_cross_entropy_lowres_bwd_workspace(B, K, hi, wi, ho, wo) > 0
    assert tiles == (K <= 8)
    return ("tile", "gather") if tiles else ("gather",)


def check_forms(shape, kw, tgt=None):
    """Every backward form the shape can take (K <= 8: tile and gather; more: gather), each against torch and the materialised
    path, then against each other; the class itself takes the tile form where there is one."""
    forms = forms_of(shape)
    got = {f: check_lowres(shape, f, tgt, **kw) for f in forms}
    base_loss, base_grad = got["gather"]
    for f in forms[:-1]:
        assert torch.equal(got[f][0], base_loss), "the forms share the forward"
        grad_close(got[f][1], base_grad, f"{shape} {f} vs gather backward")
    B, K, hi, wi, ho, wo = shape
    a = (rnd(B, hi, wi, K, seed=3) * 2.0).to(DEV).requires_grad_(True)
    y = (make_target((B, ho, wo), K, kw.get("ignore_index", -100), seed=4) if tgt is None else tgt).to(DEV)
    loss = gnn.CrossEntropyLoss(**kw).to(DEV)(gnn.LowresLogits(a, (ho, wo)), y[:, None])
    (UP * loss).backward()
    assert torch.equal(loss.detach(), base_loss) and torch.equal(a.grad, got[forms[0]][1])


# ------------------------------------------------------------------------------------------------ full resolution
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("ignore", [None, -100, 255])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("weighted", [False, True], ids=["noweight", "weight"])
@pytest.mark.parametrize("K", [2, 5, 16, 19])
def test_full_resolution(K, weighted, eps, ignore, reduction):
    B, H, W = 2, 37, 41
    logits = rnd(B, K, H, W, seed=K) * 2
    y = make_target((B, H, W), K, ignore)
    if ignore is not None:
        assert 0.1 < (y == ignore).float().mean().item() < 0.3
    kw = dict(weight=class_weights(K) if weighted else None, ignore_index=ignore, reduction=reduction, label_smoothing=eps)
    assert not weighted or ((kw["weight"] == 0).sum().item() == 1 and (y == 2 % K).any()), "one zero-weight class, present"
    loss, grad = check_full(logits, y, **kw)
    if ignore is not None:
        gi = grad.cpu().permute(0, 2, 3, 1)[y == ignore]
        assert gi.numel() > 0 and (gi == 0).all(), "the gradient of an ignored pixel is exactly 0 in every class"
    # an un-squeezed [B, 1, H, W] mask gives the same bits
    crit = gnn.CrossEntropyLoss(**kw).to(DEV)
    a = logits.to(DEV).requires_grad_(True)
    l4 = crit(a, y[:, None].to(DEV))
    (UP * l4).backward()
    assert torch.equal(l4.detach(), loss.detach()) and torch.equal(a.grad, grad)


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
    kw = dict(weight=class_weights(K), label_smoothing=0.1)
    loss, grad = check_full(logits, bad, ref_target=want, **kw)
    assert (grad.cpu().permute(0, 2, 3, 1)[pick < 0.12] == 0).all()
    check_full(logits, bad, ref=cross_entropy_ref, **kw)      # the restatement encodes the rule itself
    crit = gnn.CrossEntropyLoss(**kw).to(DEV)
    a = logits.to(DEV).requires_grad_(True)
    same = crit(a, want.to(DEV))
    (UP * same).backward()
    assert torch.equal(same.detach(), loss.detach()) and torch.equal(a.grad, grad), "the same target with those pixels ignored"


@pytest.mark.parametrize("how", ["all_ignored", "all_zero_weight"])
@pytest.mark.parametrize("K", [5, 19])
def test_zero_divisor_gives_zero_loss_and_zero_gradient(K, how):
    """D == 0 with reduction "mean": loss 0, every gradient exactly 0, nothing non-finite -- full resolution and every
    low-resolution form.  (With "sum" and label smoothing the zero-weight pixels keep their smoothing term.)"""
    B, H = 2, 32
    w = class_weights(K)
    fill = 255 if how == "all_ignored" else 2
    y = torch.full((B, H, H), fill, dtype=torch.int64)
    y[0, 0, :5] = 255      # a few ignored pixels in either case
    kw = dict(weight=w, ignore_index=255, label_smoothing=0.1)
    logits = rnd(B, K, H, H) * 2
    loss, grad = check_full(logits, y, ref=cross_entropy_ref, **kw)
    assert loss.item() == 0.0 and (grad == 0).all()
    if how == "all_zero_weight":
        loss, grad = check_full(logits, y, reduction="sum", **kw)
        assert loss.item() > 0.0 and (grad.cpu().permute(0, 2, 3, 1)[y == 255] == 0).all()
    if K <= 16:
        crit = gnn.CrossEntropyLoss(**kw).to(DEV)
        opt, up = crit._options(K), torch.tensor(UP, device=DEV)
        low, yd = (rnd(B, 9, 9, K) * 2).to(DEV), y.to(DEV)
        for form in forms_of((B, K, 9, 9, H, H)):
            loss, norm = ops.cross_entropy_lowres_fwd(low, yd, (H, H), opt)
            grad = ops.cross_entropy_lowres_bwd(low, yd, (H, H), norm, up, 1.0, opt, form=form)
            assert loss.item() == 0.0 and norm.item() == 0.0 and (grad == 0).all(), form
        a = low.clone().requires_grad_(True)
        loss = crit(gnn.LowresLogits(a, (H, H)), yd)
        (UP * loss).backward()
        assert loss.item() == 0.0 and (a.grad == 0).all()


@pytest.mark.parametrize("K", [5, 19])
def test_large_logits_stay_finite(K):
    B, H, W = 2, 21, 23
    g = torch.Generator().manual_seed(5)
    logits = (torch.randint(0, 2, (B, K, H, W), generator=g).float() * 2 - 1) * 1.0e4      # every logit is +1e4 or -1e4
    y = make_target((B, H, W), K, 255)
    for reduction in ("mean", "sum"):
        check_full(logits, y, weight=class_weights(K), ignore_index=255, reduction=reduction, label_smoothing=0.1)


# ------------------------------------------------------------------------------------------------ low resolution
LOWRES_KW = [dict(), dict(weight=True, label_smoothing=0.1, ignore_index=255), dict(weight=True, reduction="sum", ignore_index=None)]


def _kw(kw, K):
    return {**kw, "weight": class_weights(K)} if kw.get("weight") else dict(kw)


@pytest.mark.parametrize("kw", LOWRES_KW, ids=["defaults", "weight_smooth_ignore255", "weight_sum_noignore"])
@pytest.mark.parametrize("shape", LOWRES_SHAPES)
def test_low_resolution(shape, kw):
    check_forms(shape, _kw(kw, shape[1]))


@pytest.mark.parametrize("ignore", [255, None], ids=["ignored", "none_ignored"])
@pytest.mark.parametrize("shape", SKELETON_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_low_resolution_at_the_tile_edges(shape, ignore):
    """The shapes of tests/test_hip_soft_ce.py::test_low_resolution_at_the_tile_edges, with weights and smoothing; with ``ignore``
    the whole first 32 x 64 tile of image 0 is ignored."""
    check_forms(shape, dict(weight=class_weights(shape[1]), label_smoothing=0.1, ignore_index=ignore), _sce.skeleton_target(shape, ignore))


def test_low_resolution_out_of_range_target():
    B, K, hi, ho = 2, 5, 9, 32
    low = (rnd(B, hi, hi, K, seed=3) * 2).to(DEV)
    y = make_target((B, ho, ho), K, -100, seed=4)
    bad, want = y.clone(), y.clone()
    bad[:, :3] = K + 2
    want[:, :3] = -100
    crit = gnn.CrossEntropyLoss(weight=class_weights(K), label_smoothing=0.1).to(DEV)
    opt, up = crit._options(K), torch.tensor(UP, device=DEV)
    for form in ("tile", "gather"):
        la, na = ops.cross_entropy_lowres_fwd(low, bad.to(DEV), (ho, ho), opt)
        lb, nb = ops.cross_entropy_lowres_fwd(low, want.to(DEV), (ho, ho), opt)
        ga = ops.cross_entropy_lowres_bwd(low, bad.to(DEV), (ho, ho), na, up, 1.0, opt, form=form)
        gb = ops.cross_entropy_lowres_bwd(low, want.to(DEV), (ho, ho), nb, up, 1.0, opt, form=form)
        assert torch.equal(la, lb) and torch.equal(na, nb) and torch.equal(ga, gb), form


@pytest.mark.parametrize("case", ["K19", "downsample"])
def test_shapes_outside_the_kernel_limits_materialise(case):
    """More than 16 classes, or a downsample, is not a shape gdl_cross_entropy_lowres_* take: the class resizes first and runs the
    full-resolution kernels."""
    K, hi, ho = (19, 9, 32) if case == "K19" else (5, 12, 8)
    low = (rnd(2, hi, hi, K) * 2).to(DEV).requires_grad_(True)
    y = make_target((2, ho, ho), K, 255).to(DEV)
    assert not ops.cross_entropy_lowres_ok(low, (ho, ho))
    kw = dict(weight=class_weights(K), ignore_index=255, label_smoothing=0.1)
    lr = low.detach().double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    ref = torch_ref(F.interpolate(lr, size=(ho, ho), mode="bilinear", align_corners=False), y.cpu(), **kw)
    (UP * ref).backward()
    loss = gnn.CrossEntropyLoss(**kw).to(DEV)(gnn.LowresLogits(low, (ho, ho)), y)
    (UP * loss).backward()
    loss_close(loss.item(), ref.item(), LOSS_TOL_LOWRES, f"materialised {case}")
    grad_close(low.grad.permute(0, 3, 1, 2), lr.grad, f"materialised {case}")


def test_non_f32_and_non_contiguous_logits_are_upcast():
    B, K, H, W = 2, 5, 20, 24
    logits, y = rnd(B, K, H, W) * 2, make_target((B, H, W), K, 255).to(DEV)
    crit = gnn.CrossEntropyLoss(weight=class_weights(K), ignore_index=255).to(DEV)
    want = crit(logits.to(DEV), y)
    nhwc = logits.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)
    assert not nhwc.is_contiguous() and torch.equal(crit(nhwc, y), want)
    half = logits.to(DEV).bfloat16()
    assert torch.equal(crit(half, y), crit(half.float(), y))


# ------------------------------------------------------------------------------------------------ determinism, accumulation, errors
def test_two_calls_give_the_same_bits():
    up = torch.tensor(UP, device=DEV)
    for K in (5, 19):
        opt = ops.CrossEntropyOptions(0.1, 255, True, class_weights(K).to(DEV))
        logits, y = (rnd(4, K, 67, 129) * 2).to(DEV), make_target((4, 67, 129), K, 255).to(DEV)
        runs = []
        for _ in range(2):
            loss, norm = ops.cross_entropy_fwd(logits, y, opt)
            runs.append((loss, norm, ops.cross_entropy_bwd(logits, y, norm, up, 1.0, opt)))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), K
    for shape in LOWRES_SHAPES:
        B, K, hi, wi, ho, wo = shape
        opt = ops.CrossEntropyOptions(0.1, 255, True, class_weights(K).to(DEV))
        low, y = (rnd(B, hi, wi, K, seed=3) * 2).to(DEV), make_target((B, ho, wo), K, 255, seed=4).to(DEV)
        for form in forms_of(shape):
            runs = []
            for _ in range(2):
                loss, norm = ops.cross_entropy_lowres_fwd(low, y, (ho, wo), opt)
                runs.append((loss, norm, ops.cross_entropy_lowres_bwd(low, y, (ho, wo), norm, up, 1.0, opt, form=form)))
            assert all(torch.equal(a, b) for a, b in zip(*runs)), (shape, form)


def test_a_null_weight_is_all_ones():
    """The same bits without a weight pointer and with a weight tensor of ones, in every kernel family."""
    up = torch.tensor(UP, device=DEV)
    for K in (5, 19):
        logits, y = (rnd(2, K, 37, 41) * 2).to(DEV), make_target((2, 37, 41), K, 255).to(DEV)
        runs = []
        for w in (None, torch.ones(K, device=DEV)):
            opt = ops.CrossEntropyOptions(0.1, 255, True, w)
            loss, norm = ops.cross_entropy_fwd(logits, y, opt)
            runs.append((loss, norm, ops.cross_entropy_bwd(logits, y, norm, up, 1.0, opt)))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), K
    for shape in ((2, 5, 9, 9, 32, 32), (3, 16, 6, 10, 50, 41)):
        B, K, hi, wi, ho, wo = shape
        low, y = (rnd(B, hi, wi, K, seed=3) * 2).to(DEV), make_target((B, ho, wo), K, 255, seed=4).to(DEV)
        for form in forms_of(shape):
            runs = []
            for w in (None, torch.ones(K, device=DEV)):
                opt = ops.CrossEntropyOptions(0.1, 255, True, w)
                loss, norm = ops.cross_entropy_lowres_fwd(low, y, (ho, wo), opt)
                runs.append((loss, norm, ops.cross_entropy_lowres_bwd(low, y, (ho, wo), norm, up, 1.0, opt, form=form)))
            assert all(torch.equal(a, b) for a, b in zip(*runs)), (shape, form)


def test_backward_accumulates_into_an_existing_gradient():
    up = torch.tensor(UP, device=DEV)
    for K in (5, 19):
        opt = ops.CrossEntropyOptions(0.1, 255, True, class_weights(K).to(DEV))
        logits, y = (rnd(2, K, 20, 20) * 2).to(DEV), make_target((2, 20, 20), K, 255).to(DEV)
        _, norm = ops.cross_entropy_fwd(logits, y, opt)
        g = ops.cross_entropy_bwd(logits, y, norm, up, 0.5, opt)
        acc = torch.ones_like(logits)
        ops.cross_entropy_bwd(logits, y, norm, up, 0.5, opt, out=acc, accumulate=True)
        assert torch.equal(acc, 1.0 + g), K
    a = (rnd(2, 5, 20, 20) * 2).to(DEV).requires_grad_(True)
    crit, yd = gnn.CrossEntropyLoss(), make_target((2, 20, 20), 5).to(DEV)
    crit(a, yd).backward()
    first = a.grad.clone()
    crit(a, yd).backward()
    assert torch.equal(a.grad, first + first)


def test_c_entry_points_return_error_codes():
    lib = gdlhip._lib.load()
    B, K, H = 1, 3, 4

    def p(t):
        return None if t is None else t.data_ptr()
    logits, y = torch.zeros(B, K, H, H, device=DEV), torch.zeros(B, H, H, dtype=torch.int64, device=DEV)
    low = torch.zeros(B, 2, 2, K, device=DEV)
    loss, norm, grad, dlow = torch.zeros((), device=DEV), torch.ones(1, device=DEV), torch.zeros_like(logits), torch.zeros_like(low)
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)
    nb = ws.numel() * 8
    assert lib.gdl_cross_entropy_workspace(B, K, H * H) == 16 and lib.gdl_cross_entropy_lowres_workspace(B, K, H, H) == 16
    opt = (None, 0.1, 1, 255, 1)
    INVALID = -1

    def fwd(logits_=logits, y_=y, K_=K, opt_=opt, loss_=loss, norm_=norm, ws_=p(ws), nb_=nb):
        return lib.gdl_cross_entropy_fwd(p(logits_), p(y_), B, K_, H * H, *opt_, p(loss_), p(norm_), ws_, nb_, None)

    def bwd(logits_=logits, K_=K, opt_=opt, norm_=norm, grad_=grad):
        return lib.gdl_cross_entropy_bwd(p(logits_), p(y), B, K_, H * H, *opt_, p(norm_), None, 1.0, p(grad_), 0, None)

    def lfwd(low_=low, K_=K, opt_=opt, norm_=norm, ws_=p(ws), nb_=nb, size=(H, H)):
        return lib.gdl_cross_entropy_lowres_fwd(p(low_), p(y), B, K_, 2, 2, *size, *opt_, p(loss), p(norm_), ws_, nb_, None)

    def lbwd(low_=low, K_=K, opt_=opt, norm_=norm, dlow_=dlow, form=0, size=(H, H)):
        return lib.gdl_cross_entropy_lowres_bwd(p(low_), p(y), B, K_, 2, 2, *size, *opt_, p(norm_), None, 1.0, p(dlow_), None, 0, form, None)

    assert fwd() == 0 and bwd() == 0 and lfwd() == 0 and lbwd() == 0
    torch.cuda.synchronize()
    # null pointers
    assert fwd(logits_=None) == INVALID and fwd(y_=None) == INVALID and fwd(loss_=None) == INVALID and fwd(norm_=None) == INVALID
    assert fwd(ws_=None) == INVALID and bwd(logits_=None) == INVALID and bwd(norm_=None) == INVALID and bwd(grad_=None) == INVALID
    assert lfwd(low_=None) == INVALID and lfwd(norm_=None) == INVALID and lfwd(ws_=None) == INVALID
    assert lbwd(low_=None) == INVALID and lbwd(norm_=None) == INVALID and lbwd(dlow_=None) == INVALID
    assert b"null pointer" in lib.gdl_last_error()
    # a small or misaligned workspace
    assert fwd(nb_=8) == INVALID and fwd(ws_=p(ws) + 4) == INVALID and lfwd(nb_=8) == INVALID and lfwd(ws_=p(ws) + 4) == INVALID
    assert b"workspace" in lib.gdl_last_error()
    # K < 1, and K > 16 from low-resolution logits
    assert fwd(K_=0) == INVALID and bwd(K_=0) == INVALID and lfwd(K_=0) == INVALID and lbwd(K_=0) == INVALID
    assert lfwd(K_=17) == INVALID and lbwd(K_=17) == INVALID
    # a bad smoothing value
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        o = (None, bad, 1, 255, 1)
        assert fwd(opt_=o) == INVALID and bwd(opt_=o) == INVALID and lfwd(opt_=o) == INVALID and lbwd(opt_=o) == INVALID
        assert b"label_smoothing" in lib.gdl_last_error()
    # a downsample, a factor above 64, an unknown form, the tile form without its workspace
    assert lfwd(size=(1, 1)) == INVALID and lbwd(size=(1, 1)) == INVALID and lfwd(size=(130, 4)) == INVALID
    assert lbwd(form=7) == INVALID and lbwd(form=2) == INVALID
    # the Python layer: a weight of the wrong length, dtype or device
    with pytest.raises(ValueError, match="weight"):
        ops.cross_entropy_fwd(logits, y, ops.CrossEntropyOptions(weight=torch.ones(K + 1, device=DEV)))
    with pytest.raises(ValueError, match="weight"):
        ops.cross_entropy_fwd(logits, y, ops.CrossEntropyOptions(weight=torch.ones(K, device=DEV, dtype=torch.float64)))
    with pytest.raises(ValueError):
        ops.cross_entropy_lowres_fwd(low, y, (H, H), ops.CrossEntropyOptions(weight=torch.ones(K)))
    with pytest.raises(ValueError, match="tile form"):      # K = 16 has no tile form
        ops.cross_entropy_lowres_bwd(torch.zeros(B, 2, 2, 16, device=DEV), y, (H, H), norm, None, form="tile")


# ------------------------------------------------------------------------------------------------ task level
def test_dofa_training_step_from_low_resolution_logits_equals_the_materialised_step(monkeypatch):
    """One SegmentationDOFA training step on the tiny configuration of the task tests with weighted, smoothed CrossEntropyLoss and
    ignored pixels: the step asks the model for LowresLogits (no task code names this loss: ``reads_lowres`` drives it), its loss
    equals the step with FUSE_LOWRES_DICE off (full-resolution logits written and read) and the f64 F.cross_entropy on the
    materialised logits to the bounds test_hip_tasks.py holds a DOFA training step to (loss 1e-5; per-parameter gradient 3e-2 of
    its norm + 2e-6)."""
    w = class_weights(5)
    task = _sce._dofa_task(gnn.CrossEntropyLoss(weight=w, ignore_index=255, label_smoothing=0.1))
    assert task.loss.weight.device.type == "cuda", "the buffer moves with the task"
    dev = _sce._dofa_batch(7)
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
    want = sum(f * torch_ref(t.double().cpu(), y, w, 255, "mean", 0.1).item() for f, t in ((1.0, o.out), (0.4, o.aux)))
    print(f"dofa step: lowres {steps[True][0]:.8f} materialised {steps[False][0]:.8f} f64 reference {want:.8f}")
    assert abs(steps[True][0] - steps[False][0]) < 1e-5 and abs(steps[True][0] - want) < 1e-5
    assert len(steps[True][1]) > 30 and steps[True][1].keys() == steps[False][1].keys()
    for n, ga in steps[True][1].items():
        gb = steps[False][1][n]
        assert torch.isfinite(ga).all().item(), n
        err, rn = (ga - gb).norm().item(), gb.norm().item()
        assert err <= 3e-2 * rn + 2e-6, (n, err, rn)
    assert any(g_.abs().max().item() > 0 for g_ in steps[True][1].values())


def test_graphed_train_step_reproduces_the_eager_losses_bit_for_bit():
    """GraphedTrainStep (hipGraph capture of forward + weighted mean CrossEntropyLoss from low-resolution logits + backward + Adam)
    on the tiny DOFA task: one capture and three replays on batches whose ignored fraction differs, so the divisor D changes from
    replay to replay, against the same steps run eagerly, bit for bit -- a divisor baked in at capture time fails this.  In a
    process of its own (tests/_loss_graph_worker.py, scenario "cross_entropy"), one capture scenario per process as
    tests/_graph_interleave_worker.py explains."""
    worker = Path(__file__).with_name("_loss_graph_worker.py")
    run = subprocess.run([sys.executable, str(worker), "cross_entropy"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    print(res)
    assert len(res["eager"]) == 3 and res["eager"] == res["graphed"], res
    assert len(set(res["ignored"])) == 3 and len(set(res["eager"])) == 3, "the batches differ in their ignored fraction"
