"""gdlhip.nn.SoftBCEWithLogitsLoss on the GPU: the gdl_soft_bce_* kernels at full resolution (any channel count, int64 and f32
targets) and from the one-class head's low-resolution map (gather and tile backward forms), the class's routing, a one-class
DOFA task with the path on and off, a UNet++ task step with the float mask, and a captured step.

The reference is ``soft_bce_ref`` (tests/test_soft_bce_host.py): the closed form in f64 on the CPU, gradients from torch autograd;
for the low-resolution kernels it is applied to ``F.interpolate(low, size, "bilinear", align_corners=False)``.  smp is not
installed, so parity with smp itself stays unpinned.  Tolerances are those of tests/test_hip_soft_ce.py and
tests/test_hip_binary_lowres.py: loss within 1e-6 max(1, |ref|) (2e-6 from low-resolution logits), gradients within
1e-4 max|ref|; every comparison prints the error it measured."""

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


H = _load("test_soft_bce_host")
soft_bce_ref = H.soft_bce_ref
T = _load("test_hip_binary_lowres")      # SHAPES, make_inputs, forms_of, loss_close, grad_close and the tiny one-class DOFA task
Criterion = gnn.SoftBCEWithLogitsLoss      # (without the feature: AttributeError here, every test of this file fails)

DEV = "cuda"
UP = T.UP
LOSS_TOL, LOSS_TOL_LOWRES = T.LOSS_TOL, T.LOSS_TOL_LOWRES
loss_close, grad_close = T.loss_close, T.grad_close

# odd sizes that leave a ragged last workgroup; C > 1 with per-channel weights
FULL_SHAPES = [(2, 1, 37, 41), (1, 3, 16, 16), (3, 2, 5, 7)]
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def dev_options(kw):
    """ops.SoftBCEOptions on the device for the keyword arguments of soft_bce_ref."""
    return ops.SoftBCEOptions(kw["smooth_factor"], kw["ignore_index"], kw["reduction"] == "mean",
                              None if kw["weight"] is None else kw["weight"].to(DEV).contiguous(),
                              None if kw["pos_weight"] is None else kw["pos_weight"].to(DEV).contiguous())


def criterion(kw):
    return Criterion(weight=kw["weight"], ignore_index=kw["ignore_index"], reduction=kw["reduction"],
                     smooth_factor=kw["smooth_factor"], pos_weight=kw["pos_weight"]).to(DEV)


def full_reference(x, y, kw):
    """(f64 loss, UP * d loss / d x) on the CPU."""
    a = x.double().requires_grad_(True)
    ref = soft_bce_ref(a, y, **kw)
    (UP * ref).backward()
    return ref.item(), a.grad


# ------------------------------------------------------------------------------------------------ full resolution
@pytest.mark.parametrize("o", H.GRID, ids=H.grid_id)
@pytest.mark.parametrize("float_target", [False, True], ids=["int64", "f32"])
@pytest.mark.parametrize("shape", FULL_SHAPES, ids=_ids)
def test_full_resolution_loss_and_gradient(shape, float_target, o):
    """The op wrappers and the class against the f64 reference: the option grid of the host test, logits that include +-50."""
    kw = H.options_of(o, shape[1])
    x, y = H.make_case(shape, float_target, o["ignore_index"], seed=1)
    assert y.dtype == (torch.float32 if float_target else torch.int64)
    if float_target:
        assert ((y > 0) & (y < 1)).any(), "fractional target values"
    ref_loss, ref_grad = full_reference(x, y, kw)
    what = f"{shape} {'f32' if float_target else 'int64'} {H.grid_id(o)}"
    xd, yd, opt = x.to(DEV), y.to(DEV), dev_options(kw)
    loss = ops.soft_bce_fwd(xd, yd, opt)
    grad = ops.soft_bce_bwd(xd, yd, torch.tensor(UP, device=DEV), 1.0, opt)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and grad.shape == xd.shape
    loss_close(loss.item(), ref_loss, LOSS_TOL, what)
    grad_close(grad, ref_grad, what)
    if o["ignore_index"] is not None:
        assert (grad.cpu()[y.reshape(x.shape) == o["ignore_index"]] == 0).all(), "an ignored element gets exactly 0"
    a = xd.clone().requires_grad_(True)
    la = criterion(kw)(a, yd)
    (UP * la).backward()
    assert torch.equal(la.detach(), loss) and torch.equal(a.grad, grad), "the class is the two op calls"


@pytest.mark.parametrize("float_target", [False, True], ids=["int64", "f32"])
@pytest.mark.parametrize("shape", FULL_SHAPES, ids=_ids)
def test_logits_of_80_stay_finite(shape, float_target):
    o = dict(smooth_factor=0.1, per_channel=True, ignore_index=255, reduction="mean")
    kw = H.options_of(o, shape[1])
    x, y = H.make_case(shape, float_target, 255, seed=2, scale=20.0, extreme=80.0)
    assert (x == 80).any() and (x == -80).any()
    ref_loss, ref_grad = full_reference(x, y, kw)
    xd, yd, opt = x.to(DEV), y.to(DEV), dev_options(kw)
    loss = ops.soft_bce_fwd(xd, yd, opt)
    grad = ops.soft_bce_bwd(xd, yd, torch.tensor(UP, device=DEV), 1.0, opt)
    assert torch.isfinite(loss).item() and torch.isfinite(grad).all().item()
    loss_close(loss.item(), ref_loss, LOSS_TOL, f"{shape} +-80")
    grad_close(grad, ref_grad, f"{shape} +-80")


@pytest.mark.parametrize("float_target", [False, True], ids=["int64", "f32"])
def test_accumulate_adds_onto_the_gradient_buffer(float_target):
    shape = (3, 2, 5, 7)
    kw = H.options_of(dict(smooth_factor=0.1, per_channel=True, ignore_index=255, reduction="sum"), shape[1])
    x, y = H.make_case(shape, float_target, 255, seed=4, extreme=0.0)
    _, ref_grad = full_reference(x, y, kw)
    pre = torch.randn(shape, generator=torch.Generator().manual_seed(9)) * 0.1
    out = pre.to(DEV)
    got = ops.soft_bce_bwd(x.to(DEV), y.to(DEV), torch.tensor(UP, device=DEV), 1.0, dev_options(kw), out=out, accumulate=True)
    assert got is out
    err = (out.cpu().double() - (pre.double() + ref_grad)).abs().max().item()
    print(f"accumulate: max err {err:.3e} vs scale {ref_grad.abs().max().item():.3e}")
    assert err <= T.GRAD_TOL * ref_grad.abs().max().item()
    ign = y.reshape(shape) == 255
    assert ign.any() and torch.equal(out.cpu()[ign], pre[ign]), "an ignored element adds exactly 0"


def test_other_dtypes_and_shapes_reach_the_same_kernels():
    """int32 / bool targets convert to int64, f64 / bf16 targets to f32; a [B,H,W] mask against [B,1,H,W] logits; logits without
    a channel dimension."""
    x, y = H.make_case((2, 1, 9, 11), False, None, seed=6)
    xd, yd = x.to(DEV), y.to(DEV)
    crit = Criterion(smooth_factor=0.1).to(DEV)
    base = crit(xd, yd)
    for other in (yd.int(), yd.bool(), yd.float(), yd.double(), yd.bfloat16(), yd[:, None], yd[:, None].float()):
        assert torch.equal(crit(xd, other), base), other.dtype
    assert torch.equal(crit(xd.reshape(2, -1), yd.reshape(2, -1)), base)
    with pytest.raises(ValueError, match="do not match"):
        crit(xd, yd[:1])
    with pytest.raises(ValueError, match="weight"):
        Criterion(weight=H.channel_weights(3)[0]).to(DEV)(xd, yd)


def test_a_non_finite_logit_under_an_ignored_element_does_not_poison_the_sum():
    x, y = H.make_case((2, 1, 9, 11), False, 255, seed=8)
    ign = y.reshape(x.shape) == 255
    assert ign.sum().item() >= 4
    clean_loss, clean_grad = full_reference(x, y, dict(weight=None, pos_weight=None, smooth_factor=None, ignore_index=255, reduction="mean"))
    bad = x.clone()
    where = ign.nonzero()
    bad[tuple(where[0])], bad[tuple(where[1])], bad[tuple(where[2])] = float("nan"), float("inf"), float("-inf")
    a = bad.to(DEV).requires_grad_(True)
    loss = Criterion(ignore_index=255)(a, y.to(DEV))
    (UP * loss).backward()
    loss_close(loss.item(), clean_loss, LOSS_TOL, "non-finite logits under ignored elements")
    grad_close(a.grad, clean_grad, "non-finite logits under ignored elements")
    assert (a.grad.cpu()[ign] == 0).all()


# ------------------------------------------------------------------------------------------------ low resolution
LOW_CASES = {
    "plain": dict(weight=None, pos_weight=None, smooth_factor=None, ignore_index=255, reduction="mean"),
    "smooth-weights": dict(weight=torch.tensor(0.7), pos_weight=torch.tensor([2.0]), smooth_factor=0.1, ignore_index=255, reduction="mean"),
    "smooth-sum": dict(weight=None, pos_weight=torch.tensor([[[0.5]]]), smooth_factor=0.1, ignore_index=255, reduction="sum"),
    "no-ignore": dict(weight=None, pos_weight=torch.tensor([2.0]), smooth_factor=0.1, ignore_index=None, reduction="mean"),
}


def low_inputs(shape, float_target, ignore=255):
    """``make_inputs`` of tests/test_hip_binary_lowres.py (10 % ignored at random plus the top-left ninth of image 0; it asserts the
    10-30 % share; its other pattern on T.SKELETON_SHAPES; nothing ignored with ``ignore`` None); the f32 target holds 0.25 / 0.75
    in place of 0 / 1 and 255.0 at the ignored pixels."""
    low, tgt = T.make_inputs(shape, ignore)
    if float_target:
        tgt = torch.where(tgt == 255, torch.tensor(255.0), 0.25 + 0.5 * tgt.float())
    return low, tgt


@functools.lru_cache(maxsize=None)
def low_reference(shape, case, float_target):
    """(low, target, f64 loss, UP * d loss / d low [B,hi,wi,1], dead): computed once, never modified.  ``dead`` marks the
    low-resolution logits whose every contributing pixel is ignored (from the resize's own weights)."""
    kw = LOW_CASES[case]
    low, tgt = low_inputs(shape, float_target, kw["ignore_index"])
    size = shape[3:]
    lr = low.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = soft_bce_ref(F.interpolate(lr, size=size, mode="bilinear", align_corners=False), tgt, **kw)
    (UP * ref).backward()
    w = low.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    valid = (tgt != 255).double()[:, None]
    (F.interpolate(w, size=size, mode="bilinear", align_corners=False) * valid).sum().backward()
    dead = (w.grad == 0).permute(0, 2, 3, 1)
    return low, tgt, ref.item(), lr.grad.permute(0, 2, 3, 1).contiguous(), dead


def run_low(opt, low, tgt, size, form, up=UP):
    return (ops.soft_bce_lowres_fwd(low, tgt, size, opt),
            ops.soft_bce_lowres_bwd(low, tgt, size, torch.tensor(up, device=DEV), 1.0, opt, form=form))


@pytest.mark.parametrize("float_target", [False, True], ids=["int64", "f32"])
@pytest.mark.parametrize("case", list(LOW_CASES))
@pytest.mark.parametrize("shape", T.SHAPES + T.SKELETON_SHAPES, ids=_ids)
def test_loss_and_gradient_from_the_low_resolution_map(shape, case, float_target):
    """Every backward form the shape admits, against the f64 reference and against the class's own materialised route; the class
    itself takes the low-resolution node (``upsample_logits`` is never called) up to factor 8 and materialises beyond it."""
    kw = LOW_CASES[case]
    low, tgt, ref_loss, ref_grad, dead = low_reference(shape, case, float_target)
    size = tuple(shape[3:])
    crit, opt = criterion(kw), dev_options(kw)
    lowd, tgtd = low.to(DEV), tgt.to(DEV)
    b_ = lowd.clone().requires_grad_(True)
    lb = crit(gnn.LowresLogits(b_, size).materialise(), tgtd)
    (UP * lb).backward()
    forms = T.forms_of(shape)
    got = {}
    for form in forms:
        what = f"{case} {shape} {'f32' if float_target else 'int64'} {form}"
        loss, grad = run_low(opt, lowd, tgtd, size, form)
        assert loss.dim() == 0 and torch.isfinite(loss).item() and torch.isfinite(grad).all().item()
        loss_close(loss.item(), ref_loss, LOSS_TOL_LOWRES, what)
        loss_close(loss.item(), lb.item(), LOSS_TOL, what + " vs the materialised route")
        grad_close(grad, ref_grad, what + " vs torch")
        grad_close(grad, b_.grad, what + " vs the materialised route")
        if dead.any():
            assert (grad.cpu()[dead] == 0).all(), what + ": a logit whose every contributing pixel is ignored gets exactly 0"
        got[form] = (loss, grad)
    if shape[1] >= 5 and kw["ignore_index"] is not None:
        assert dead.any()
    for form in forms[:-1]:
        assert torch.equal(got[form][0], got["gather"][0]), "the forms share the forward"
        grad_close(got[form][1], got["gather"][1], f"{case} {shape} {form} vs gather")
    auto = ops.soft_bce_lowres_bwd(lowd, tgtd, size, torch.tensor(UP, device=DEV), 1.0, opt)
    assert torch.equal(auto, got[forms[0]][1]), "auto is the tile form where the shape takes it"
    calls, mats = [], []
    real_up, real_mat = ops.upsample_logits, gnn.LowresLogits.materialise
    ops.upsample_logits = lambda *a, **k: calls.append(1) or real_up(*a, **k)
    gnn.LowresLogits.materialise = lambda self: mats.append(1) or real_mat(self)
    try:
        a = lowd.clone().requires_grad_(True)
        la = crit(gnn.LowresLogits(a, size), tgtd)
        (UP * la).backward()
    finally:
        ops.upsample_logits, gnn.LowresLogits.materialise = real_up, real_mat
    factor = max(-(-shape[3] // shape[1]), -(-shape[4] // shape[2]))
    assert ops.binary_lowres_pays(lowd, size) == (factor <= 8)
    if factor <= 8:
        assert calls == [] and mats == [], "the class reads the low-resolution map"
        assert torch.equal(la.detach(), got[forms[0]][0]) and torch.equal(a.grad, got[forms[0]][1])
    else:      # beyond ops.BINARY_LOWRES_MAX_FACTOR the class materialises and takes the full-resolution node
        assert calls == [1] and mats == [1] and torch.equal(la.detach(), lb.detach()) and torch.equal(a.grad, b_.grad)


def test_the_class_materialises_when_the_path_is_off_or_the_batch_sizes_differ(monkeypatch):
    shape = T.SHAPES[0]
    low, tgt = (t.to(DEV) for t in low_inputs(shape, False))
    size = tuple(shape[3:])
    crit = Criterion(ignore_index=255)
    want = crit(gnn.LowresLogits(low, size), tgt)
    calls = []
    real = ops.upsample_logits
    monkeypatch.setattr(ops, "upsample_logits", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", False)
    off = crit(gnn.LowresLogits(low, size), tgt)
    assert calls == [1]
    loss_close(off.item(), want.item(), LOSS_TOL, "path off vs on")
    monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", True)
    with pytest.raises(ValueError, match="do not match"):
        crit(gnn.LowresLogits(low, size), tgt[:1])


# ------------------------------------------------------------------------------------------------ edge targets
@pytest.mark.parametrize("float_target", [False, True], ids=["int64", "f32"])
def test_all_zero_all_one_and_all_ignored_targets(float_target):
    """All-zero and all-one targets against the reference (BCE is positive for every finite logit: neither is 0); every element
    ignored: loss exactly 0 and gradient exactly 0, at full resolution and in both low-resolution forms."""
    dt = torch.float32 if float_target else torch.int64
    kw = dict(weight=None, pos_weight=torch.tensor(1.5), smooth_factor=0.1, ignore_index=255, reduction="mean")
    opt = dev_options(kw)
    full = (2, 1, 37, 41)
    x = H.make_case(full, False, None, seed=12)[0]
    lows = [(s, T.make_inputs(s, None, seed=5)[0]) for s in T.SHAPES]
    for name, value in (("all-zero", 0), ("all-one", 1), ("all-ignored", 255)):
        y = torch.full((full[0], *full[2:]), value, dtype=dt)
        loss = ops.soft_bce_fwd(x.to(DEV), y.to(DEV), opt)
        grad = ops.soft_bce_bwd(x.to(DEV), y.to(DEV), torch.tensor(UP, device=DEV), 1.0, opt)
        if value == 255:
            assert loss.item() == 0.0 and (grad == 0).all().item(), name
        else:
            ref_loss, ref_grad = full_reference(x, y, kw)
            assert ref_loss > 0
            loss_close(loss.item(), ref_loss, LOSS_TOL, f"{name} {full}")
            grad_close(grad, ref_grad, f"{name} {full}")
        for shape, low in lows:
            size = tuple(shape[3:])
            y = torch.full((shape[0], *size), value, dtype=dt)
            if value != 255:
                lr = low.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
                ref = soft_bce_ref(F.interpolate(lr, size=size, mode="bilinear", align_corners=False), y, **kw)
                (UP * ref).backward()
            for form in T.forms_of(shape):
                loss, grad = run_low(opt, low.to(DEV), y.to(DEV), size, form)
                if value == 255:
                    assert loss.item() == 0.0 and (grad == 0).all().item(), (name, shape, form)
                else:
                    loss_close(loss.item(), ref.item(), LOSS_TOL_LOWRES, f"{name} {shape} {form}")
                    grad_close(grad, lr.grad.permute(0, 2, 3, 1), f"{name} {shape} {form}")


# ------------------------------------------------------------------------------------------------ determinism
def test_two_launches_give_the_same_bits():
    kw = H.options_of(dict(smooth_factor=0.1, per_channel=True, ignore_index=255, reduction="mean"), 3)
    opt = dev_options(kw)
    for float_target in (False, True):
        x, y = (t.to(DEV) for t in H.make_case((2, 3, 37, 41), float_target, 255, seed=3))
        up = torch.tensor(UP, device=DEV)
        runs = [(ops.soft_bce_fwd(x, y, opt), ops.soft_bce_bwd(x, y, up, 1.0, opt)) for _ in range(2)]
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        lopt = dev_options(LOW_CASES["smooth-weights"])
        for shape in T.SHAPES:
            low, tgt = (t.to(DEV) for t in low_inputs(shape, float_target))
            for form in T.forms_of(shape):
                runs = [run_low(lopt, low, tgt, tuple(shape[3:]), form) for _ in range(2)]
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), (shape, form, float_target)


# ------------------------------------------------------------------------------------------------ argument checking
def test_c_entry_points_refuse_bad_arguments_without_launching():
    """Null pointers, a too-small or misaligned workspace, an unknown target tag or form, a weight numel that is neither 1 nor C and
    low-resolution shapes outside the limits are GDL_CHECK_ARG errors (status -1).  Every output buffer keeps its sentinel: nothing
    ran."""
    import ctypes as C
    lib = gdlhip._lib.load()
    P = ops._p
    B, Cn, Hh, Ww = 2, 3, 8, 8
    x = torch.zeros(B, Cn, Hh, Ww, device=DEV)
    y = torch.zeros(B, Cn, Hh, Ww, dtype=torch.int64, device=DEV)
    w3, w2 = torch.ones(3, device=DEV), torch.ones(2, device=DEV)
    loss, dx = torch.full((), 7.0, device=DEV), torch.full_like(x, 7.0)
    nb = lib.gdl_soft_bce_workspace(B, Cn, Hh * Ww)
    assert nb >= 8 and nb % 8 == 0
    ws = torch.zeros(nb // 8 + 2, dtype=torch.float64, device=DEV)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)  # noqa: E731

    def opt(weight=None, wn=0, pos=None, pn=0, smooth=0.1, scale=1.0):
        return (1, smooth, 1, 255, 255.0, P(weight), wn, P(pos), pn, scale)

    def fwd(logits=x, target=y, tag=0, b=B, c=Cn, hw=Hh * Ww, o=None, out=loss, w=None, wbytes=nb):
        return lib.gdl_soft_bce_fwd(P(logits), P(target), tag, b, c, hw, *(o or opt()), P(out), P(ws) if w is None else w, wbytes, None)

    def bwd(logits=x, target=y, tag=0, b=B, c=Cn, hw=Hh * Ww, o=None, out=dx):
        return lib.gdl_soft_bce_bwd(P(logits), P(target), tag, b, c, hw, *(o or opt()), None, 1.0, P(out), 0, None)

    assert fwd() == 0 and bwd() == 0, "the good call, once: the arguments above are valid"
    loss.fill_(7.0), dx.fill_(7.0)
    bad_fwd = [fwd(logits=None), fwd(target=None), fwd(out=None), fwd(w=C.c_void_p(None)), fwd(wbytes=nb - 8), fwd(w=off(ws, 4)),
               fwd(tag=2), fwd(tag=-1), fwd(b=0), fwd(c=0), fwd(hw=0), fwd(o=opt(w2, 2)), fwd(o=opt(pos=w2, pn=2)),
               fwd(o=opt(w3, 3), c=2), fwd(o=opt(smooth=1.5)), fwd(o=opt(scale=0.0))]
    bad_bwd = [bwd(logits=None), bwd(target=None), bwd(out=None), bwd(tag=2), bwd(b=0), bwd(o=opt(w2, 2)), bwd(o=opt(pos=w2, pn=2)),
               bwd(o=opt(smooth=-0.5))]
    assert bad_fwd == [-1] * len(bad_fwd), bad_fwd
    assert bad_bwd == [-1] * len(bad_bwd), bad_bwd
    assert fwd(o=opt(w3, 3)) == 0 and fwd(o=opt(w3, 1, w3, 3)) == 0      # 1 or C values: taken
    loss.fill_(7.0)

    low, ly = torch.zeros(1, 8, 8, 1, device=DEV), torch.zeros(1, 32, 32, dtype=torch.int64, device=DEV)
    dlow = torch.full_like(low, 7.0)
    lnb, tnb = lib.gdl_soft_bce_lowres_workspace(1, 32, 32), lib.gdl_binary_lowres_bwd_workspace(1, 8, 8, 32, 32)
    assert lnb >= 8 and tnb > 0
    tws = torch.zeros(tnb // 4 + 2, device=DEV)

    def lfwd(lo=low, target=ly, tag=0, dims=(1, 8, 8, 32, 32), o=None, out=loss, w=None, wbytes=lnb):
        return lib.gdl_soft_bce_lowres_fwd(P(lo), P(target), tag, *dims, *(o or opt()), P(out), P(ws) if w is None else w, wbytes, None)

    def lbwd(lo=low, target=ly, tag=0, dims=(1, 8, 8, 32, 32), o=None, out=dlow, w=None, wbytes=tnb, form=2):
        return lib.gdl_soft_bce_lowres_bwd(P(lo), P(target), tag, *dims, *(o or opt()), None, 1.0, P(out), P(tws) if w is None else w,
                                           wbytes, form, None)

    bad = [lfwd(lo=None), lfwd(target=None), lfwd(out=None), lfwd(w=C.c_void_p(None)), lfwd(wbytes=lnb - 8), lfwd(w=off(ws, 4)),
           lfwd(tag=2), lfwd(o=opt(w3, 3)), lfwd(o=opt(pos=w2, pn=2)),
           lbwd(lo=None), lbwd(target=None), lbwd(out=None), lbwd(w=C.c_void_p(None)), lbwd(wbytes=tnb - 4), lbwd(w=off(tws, 2)),
           lbwd(tag=2), lbwd(form=3), lbwd(form=-1), lbwd(o=opt(w3, 3)),
           lbwd(dims=(1, 8, 8, 8, 8)), ]      # (the tile form on a 1:1 map)
    for hi, wi, ho, wo in ((8, 8, 4, 8), (8, 8, 8, 4), (1, 1, 65, 8), (1, 1, 8, 65), (0, 8, 8, 8)):
        bad += [lfwd(dims=(1, hi, wi, ho, wo)), lbwd(dims=(1, hi, wi, ho, wo), form=0)]
    bad += [lfwd(dims=(0, 8, 8, 32, 32)), lbwd(dims=(0, 8, 8, 32, 32), form=1)]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert loss.item() == 7.0 and (dx == 7.0).all().item() and (dlow == 7.0).all().item(), "nothing was launched"
    with pytest.raises(ValueError, match="tile form"):
        ops.soft_bce_lowres_bwd(low, torch.zeros(1, 8, 8, dtype=torch.int64, device=DEV), (8, 8), None, form="tile")
    with pytest.raises(ValueError, match="smooth_factor"):
        ops.soft_bce_fwd(x, y, ops.SoftBCEOptions(1.5, None, True))
    assert lbwd() == 0 and lbwd(form=1, w=C.c_void_p(None), wbytes=0) == 0, "the good calls: the arguments above are valid"
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ task level
def test_one_class_dofa_task_with_the_path_on_and_off(monkeypatch):
    """``training_step`` and ``validation_step`` of the tiny one-class DOFA task (tests/test_hip_binary_lowres.py) with
    SoftBCEWithLogitsLoss give the same loss and gradients within this file's tolerances, and the same mask, with
    GDL_LOWRES_DICE on and off; the on-run never writes resized logits (``upsample_logits`` is not called).  The gradient bound
    1e-4 max|ref| is taken over the whole parameter gradient (a conv bias in front of a BatchNorm has a mathematically zero
    gradient: its entries are rounding noise and have no scale of their own); per parameter the bound of the existing
    on-and-off test holds as well."""
    loss = Criterion(ignore_index=255, smooth_factor=0.1, pos_weight=torch.tensor([1.5]))
    assert gnn.reads_lowres(loss, 1)
    task = T._one_class_dofa_task(loss)
    assert loss.pos_weight.is_cuda, "the buffers move with the task"
    batch = T._one_class_batch(7)
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
    print(f"upsample_logits calls on {out[True][4]} off {out[False][4]}")
    assert out[True][4] == 0 and out[False][4] == 4, "two heads, training and validation"
    loss_close(out[True][0], out[False][0], LOSS_TOL, "train loss, path on vs off")
    loss_close(out[True][1], out[False][1], LOSS_TOL, "val loss, path on vs off")
    assert out[True][0] > 0.1
    assert out[True][2].dtype == torch.int64 and out[True][2].shape == (4, T.IMG, T.IMG)
    assert torch.equal(out[True][2], out[False][2])
    print(f"share of ones in the mask: {out[True][2].float().mean().item():.4f}")
    assert len(out[True][3]) > 30 and out[True][3].keys() == out[False][3].keys()
    names = sorted(out[True][3])
    grad_close(torch.cat([out[True][3][n].reshape(-1) for n in names]), torch.cat([out[False][3][n].reshape(-1) for n in names]),
               "every parameter gradient, path on vs off")
    for n in names:
        ga, gb = out[True][3][n], out[False][3][n]
        err, rn = (ga - gb).norm().item(), gb.norm().item()
        assert err <= 3e-2 * rn + 2e-6, (n, err, rn)
    assert any(g_.abs().max().item() > 0 for g_ in out[True][3].values())


def test_one_class_unetplus_step_with_the_float_mask_matches_the_oracle():
    """SegmentationUnetPlus hands the float ``[B,1,H,W]`` mask to the loss as it is (the f32-target kernels).  The loss kernel is
    held to this file's tolerances on the task's own logits; the whole step is held against oracle/unetpp.py + ``soft_bce_ref``
    to the bounds every UNet++ step-versus-oracle test of the suite uses (loss 1e-5, per-parameter gradient 3e-2 of its norm +
    2e-6: tests/test_hip_soft_ce.py::test_quickstart_shaped_unetplus_step_matches_the_oracle), which measure the f32 model, not
    the loss."""
    from geo_deep_learning.tasks_with_models.segmentation_unetplus import SegmentationUnetPlus
    from oracle import procedural_state_dict, synthetic_batch
    from oracle.unetpp import UnetPlusPlus as OracleUnetPlusPlus
    S = _load("test_hip_soft_ce")
    seed, b = 9, 2
    kw = dict(weight=None, pos_weight=torch.tensor([2.0]), smooth_factor=0.1, ignore_index=255, reduction="mean")
    ora = OracleUnetPlusPlus("resnet18", 3, 1)
    sd = procedural_state_dict(ora, seed)
    ora.load_state_dict(sd)
    task = SegmentationUnetPlus("resnet18", (128, 128), 3, 1, max_samples=2, loss=criterion(kw))
    task.configure_model()
    task.model.load_state_dict(sd)
    task = task.to(DEV)
    batch = synthetic_batch(b, 3, 128, 2, seed)
    mask = batch["mask"] = batch["mask"].float()      # the reference's datamodule hands out float masks
    assert mask.shape == (b, 1, 128, 128) and set(mask.unique().tolist()) == {0.0, 1.0}
    mask[torch.rand(mask.shape, generator=torch.Generator().manual_seed(2)) < 0.1] = 255.0
    dev = {k: (v.to(DEV) if isinstance(v, torch.Tensor) and k != "wavelengths" else v) for k, v in batch.items()}

    class _Trainer:
        training, datamodule, estimated_stepping_batches, accumulate_grad_batches, max_epochs = True, None, 100, 1, 3
    task.trainer = _Trainer()
    seen = []
    real = ops.soft_bce_fwd
    ops.soft_bce_fwd = lambda logits, target, options: seen.append((logits.detach().clone(), target.dtype)) or real(logits, target, options)
    try:
        task.train(); ora.train()
        loss = task.training_step(dev, 0)
        loss.backward()
    finally:
        ops.soft_bce_fwd = real
    assert len(seen) == 1 and seen[0][1] == torch.float32, "the float mask reaches the f32-target kernel unconverted"
    loss_close(loss.item(), soft_bce_ref(seen[0][0].cpu(), mask, **kw).item(), LOSS_TOL, "unet++ loss on the task's own logits")
    lo = soft_bce_ref(ora(batch["image"]), mask, **kw)
    lo.backward()
    print(f"unet++ one-class step: loss {loss.item():.8f} oracle {lo.item():.8f}")
    assert abs(loss.item() - lo.item()) < 1e-5
    assert S._param_grads_close(task.model, ora) > 100


def test_graphed_soft_bce_step_reproduces_the_eager_losses_bit_for_bit():
    """GraphedTrainStep (hipGraph capture of forward + SoftBCEWithLogitsLoss from the one-class low-resolution maps + backward +
    Adam): one capture and three replays against the same steps run eagerly, bit for bit.  In a fresh child process
    (tests/_loss_graph_worker.py, scenario "soft_bce") under its own time limit; nothing follows a non-zero exit status."""
    worker = Path(__file__).with_name("_loss_graph_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(worker), "soft_bce"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    print(res)
    assert len(res["eager"]) == 3 and res["eager"] == res["graphed"], res
    assert res["upsample_logits_calls"] == 0
