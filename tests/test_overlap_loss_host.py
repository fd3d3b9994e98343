"""gdlhip.nn.JaccardLoss and TverskyLoss, the parts that need no GPU: constructor contract, the config aliases, the
``reads_lowres`` predicate, the ctypes mirror of gdl_overlap_options, and the reference restatement the GPU tests
(test_hip_overlap_loss.py) hold the kernels against.

Reference: ``overlap_ref`` below, the formulas of the class docstrings in plain torch ops (f64 in every comparison, gradients
from autograd).  smp is not available, so parity with smp itself is unpinned; what is pinned here is that the restatement with
``alpha = beta = 0.5, gamma = 1, smooth = 0`` is the Dice restatement of test_hip_dice_options.py, and that Jaccard is
``d / (2 - d)`` of the per-class Dice score."""

import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402


def overlap_ref(logits, target, kind, mode="multiclass", ignore_index=None, smooth=0.0, log_loss=False, classes=None,
                alpha=0.5, beta=0.5, gamma=1.0, eps=1e-7):
    """Jaccard / Tversky / Dice (``kind``) in the dtype of ``logits``: (loss, score_k, Y_k, m).  Masking by ``ignore_index`` as
    dice_ref of test_hip_dice_options.py; ``m`` is the class mean before ``** gamma``."""
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
    if kind == "dice":
        num, den = 2.0 * inter + smooth, psum + ysum + smooth
    elif kind == "jaccard":
        num, den = inter + smooth, psum + ysum - inter + smooth
    else:
        assert kind == "tversky"
        num, den = inter + smooth, inter + alpha * (psum - inter) + beta * (ysum - inter) + smooth
    score = num / den.clamp_min(eps)
    loss = -torch.log(score.clamp_min(eps)) if log_loss else 1.0 - score
    loss = loss * (ysum > 0).to(p.dtype)
    if classes is not None:
        loss = loss[list(classes)]
    m = loss.mean()
    return (m ** gamma if kind == "tversky" else m), score.detach(), ysum.detach(), m.detach()


def _inputs(seed=0, k=5, ignore=None):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(2, k, 12, 14, generator=g) * 2).double()
    y = torch.randint(0, k - 1, (2, 12, 14), generator=g)       # class k-1 absent
    if ignore is not None:
        y[torch.rand(y.shape, generator=g) < 0.25] = ignore
    return x, y


# ------------------------------------------------------------------------------------------------ constructors
def test_jaccard_constructor_accepts_smp_arguments_and_rejects_the_rest():
    crit = gnn.JaccardLoss("multiclass")
    assert (crit.mode, crit.classes, crit.log_loss, crit.smooth, crit.eps) == ("multiclass", None, False, 0.0, 1e-7)
    assert crit.options == ops.OverlapOptions("jaccard")
    crit = gnn.JaccardLoss(mode="multiclass", classes=[1, 3], log_loss=True, from_logits=True, smooth=1.0, eps=1e-6)
    assert crit.options == ops.OverlapOptions("jaccard", None, 1.0, True, (1, 3)) and crit.eps == 1e-6
    assert gnn.JaccardLoss(mode="binary", classes=[0]).options.classes == (0,)
    with pytest.raises(TypeError):
        gnn.JaccardLoss(ignore_index=255)          # smp's JaccardLoss has no ignore_index
    with pytest.raises(NotImplementedError):
        gnn.JaccardLoss(mode="multilabel")
    with pytest.raises(NotImplementedError):
        gnn.JaccardLoss(from_logits=False)
    for bad in ([], [1, 1], [-1, 2]):
        with pytest.raises(ValueError):
            gnn.JaccardLoss(classes=bad)
    with pytest.raises(ValueError):
        gnn.JaccardLoss(mode="binary", classes=[1])
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gnn.JaccardLoss(smooth=bad)
    with pytest.raises(ValueError, match="out of range"):
        gnn.JaccardLoss(classes=[1, 7])(torch.zeros(1, 5, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))


def test_tversky_constructor_accepts_smp_arguments_and_rejects_the_rest():
    crit = gnn.TverskyLoss("multiclass")
    assert (crit.alpha, crit.beta, crit.gamma, crit.smooth, crit.ignore_index, crit.eps) == (0.5, 0.5, 1.0, 0.0, None, 1e-7)
    assert crit.options == ops.OverlapOptions("tversky", None, 0.0, False, None, 0.5, 0.5, 1.0)
    crit = gnn.TverskyLoss(mode="multiclass", classes=[0, 2], log_loss=True, smooth=1.0, ignore_index=255, alpha=0.3, beta=0.7,
                           gamma=0.75)
    assert crit.options == ops.OverlapOptions("tversky", 255, 1.0, True, (0, 2), 0.3, 0.7, 0.75)
    assert gnn.TverskyLoss(ignore_index=-100).options.ignore_index == -100
    assert gnn.TverskyLoss(alpha=0, beta=0).options.alpha == 0.0
    assert gnn.TverskyLoss(mode="binary", classes=[0], gamma=2).options.gamma == 2.0
    with pytest.raises(NotImplementedError):
        gnn.TverskyLoss(mode="multilabel")
    with pytest.raises(NotImplementedError):
        gnn.TverskyLoss(from_logits=False)
    for bad in ([], [1, 1], [-1, 2]):
        with pytest.raises(ValueError):
            gnn.TverskyLoss(classes=bad)
    with pytest.raises(ValueError):
        gnn.TverskyLoss(mode="binary", classes=[1])
    for bad in (2.5, True, 2**63):
        with pytest.raises(ValueError):
            gnn.TverskyLoss(ignore_index=bad)
    for key in ("smooth", "alpha", "beta", "gamma"):
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError):
                gnn.TverskyLoss(**{key: bad})
    for kw in (dict(alpha=-0.1), dict(beta=-1.0), dict(gamma=0.0), dict(gamma=-1.0)):
        with pytest.raises(ValueError):
            gnn.TverskyLoss(**kw)
    with pytest.raises(ValueError, match="out of range"):
        gnn.TverskyLoss(classes=[5])(torch.zeros(1, 5, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))


def test_ops_refuse_cpu_tensors():
    x, y = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    opt = ops.OverlapOptions("tversky")
    with pytest.raises(ValueError):
        ops.dice_loss_fwd(x, y, options=opt)
    with pytest.raises(ValueError):
        ops.dice_loss_lowres_fwd(torch.zeros(1, 2, 2, 3), y, (4, 4), options=opt)
    with pytest.raises(ValueError):
        ops.dice_binary_loss_fwd(torch.zeros(1, 1, 4, 4), y, options=opt)
    for crit in (gnn.JaccardLoss(), gnn.TverskyLoss(), gnn.JaccardLoss(mode="binary")):
        with pytest.raises(ValueError):
            crit(x[:, :1] if crit.mode == "binary" else x, y)


# ------------------------------------------------------------------------------------------------ routing
ROUTES = [(None, "gdl_dice_{}_{}"), (ops.DiceOptions(255), "gdl_dice_{}_opt_{}"), (ops.OverlapOptions("tversky", 255), "gdl_overlap_{}_{}")]


@pytest.mark.parametrize("options,pattern", ROUTES, ids=["plain", "dice-options", "overlap-options"])
def test_ops_route_options_to_the_entry_point_and_argument_positions(monkeypatch, options, pattern):
    """The one decision gdlhip.ops makes for this family: ``options`` picks the C symbol, the option pointer follows ``eps``
    (absent for None), and ``eps`` / ``grad_scale`` land on the float positions of _lib.SIGNATURES.  No library is loaded."""
    import ctypes as C

    from gdlhip import _lib
    calls = []

    class Recorder:
        """Either view of the library: a size query may go through both, a launch only through the one that checks its status."""

        def __init__(self, checks_status):
            self.checks_status = checks_status

        def __getattr__(self, name):
            if name.endswith("_workspace"):
                return lambda *a: 48
            assert self.checks_status and name in _lib.STATUS_FUNCTIONS, f"{name}: launched through the view that drops its status"
            return lambda *a: calls.append((name, a)) or 0

    monkeypatch.setattr(_lib, "load", lambda: Recorder(False))
    monkeypatch.setattr(_lib, "checked", lambda: Recorder(True))
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: 7)
    EPS, GS = 3e-5, 0.25
    x, y, low, xb = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(1, 2, 2, 3), torch.zeros(1, 1, 4, 4)
    sums, up = torch.zeros(9), torch.ones(())
    runs = [("loss", "fwd", lambda: ops.dice_loss_fwd(x, y, EPS, options=options)),
            ("loss", "bwd", lambda: ops.dice_loss_bwd(x, y, sums, up, GS, EPS, options=options)),
            ("loss_lowres", "fwd", lambda: ops.dice_loss_lowres_fwd(low, y, (4, 4), EPS, options=options)),
            ("loss_lowres", "bwd", lambda: ops.dice_loss_lowres_bwd(low, y, (4, 4), sums, up, GS, EPS, options=options)),
            ("binary_loss", "fwd", lambda: ops.dice_binary_loss_fwd(xb, y, EPS, options=options)),
            ("binary_loss", "bwd", lambda: ops.dice_binary_loss_bwd(xb, y, sums[:3], up, GS, EPS, options=options))]
    for stem, way, run in runs:
        calls.clear()
        run()
        want = pattern.format(stem, way)
        assert [c[0] for c in calls] == [want]
        args, types = calls[0][1], _lib.SIGNATURES[want][1]
        assert len(args) == len(types) and args[-1] == 7
        floats = [i for i, t in enumerate(types) if t is C.c_float]
        assert len(floats) == (1 if way == "fwd" else 2)
        assert args[floats[0]] == EPS and (way == "fwd" or args[floats[1]] == GS)
        # the option pointer is the argument after eps: one more argument than the plain symbol, a non-zero address
        plain = _lib.SIGNATURES[f"gdl_dice_{stem}_{way}"][1]
        if options is None:
            assert types is plain and isinstance(args[floats[0] + 1], C.c_void_p)      # (sums: a tensor pointer)
        else:
            assert len(types) == len(plain) + 1
            assert isinstance(args[floats[0] + 1], int) and args[floats[0] + 1] != 0


# ------------------------------------------------------------------------------------------------ wiring
@pytest.mark.parametrize("name,init,cls", [
    ("JaccardLoss", {"mode": "multiclass", "smooth": 1.0}, "JaccardLoss"),
    ("TverskyLoss", {"mode": "multiclass", "alpha": 0.3, "beta": 0.7, "gamma": 0.75, "ignore_index": 255}, "TverskyLoss")])
def test_config_alias_resolves_to_the_hip_loss(name, init, cls):
    from geo_deep_learning import train as gdl_train
    crit = gdl_train.instantiate({"class_path": f"segmentation_models_pytorch.losses.{name}", "init_args": init})
    assert type(crit) is getattr(gnn, cls)
    for k, v in init.items():
        assert getattr(crit, k) == v
    # the same spec nested in a task's init_args, as a reference yaml carries it
    node = {"class_path": "types.SimpleNamespace",
            "init_args": {"loss": {"class_path": f"segmentation_models_pytorch.losses.{name}", "init_args": init}}}
    assert type(gdl_train.instantiate(node).loss) is getattr(gnn, cls)


def test_reads_lowres_is_true_for_multiclass_and_false_for_binary():
    assert gnn.reads_lowres(gnn.JaccardLoss(mode="multiclass"))
    assert gnn.reads_lowres(gnn.TverskyLoss(mode="multiclass", alpha=0.3, beta=0.7, gamma=0.75))
    assert not gnn.reads_lowres(gnn.JaccardLoss(mode="binary"))
    assert not gnn.reads_lowres(gnn.TverskyLoss(mode="binary"))
    assert gnn.reads_lowres(gnn.DiceLoss(mode="multiclass")) and not gnn.reads_lowres(gnn.DiceLoss(mode="binary"))


def test_dofa_task_hands_tversky_low_resolution_logits(monkeypatch):
    """SegmentationDOFA, unedited, asks the model for ``lowres_logits=True`` when its loss is a multiclass TverskyLoss or
    JaccardLoss, and for the resized logits when the low-resolution path is switched off (GDL_LOWRES_DICE=0)."""
    from tasks_with_models.segmentation_dofa import SegmentationDOFA
    calls = []

    class Model(torch.nn.Module):
        def forward(self, x, wv, lowres_logits=False):
            calls.append(bool(lowres_logits))
            out = torch.zeros(x.shape[0], 5, 8, 8, requires_grad=True)
            return SimpleNamespace(out=out, aux=out)

    def fake(cls, **kw):       # the class the predicate tests for; no kernel behind it here
        return type("Fake" + cls.__name__, (cls,), {"forward": lambda self, y_pred, y_true: y_pred.sum() * 0.0})(**kw)

    batch = {"image": torch.zeros(2, 3, 8, 8), "mask": torch.zeros(2, 1, 8, 8, dtype=torch.int64),
             "wavelengths": torch.tensor([0.6, 0.5, 0.4])}
    monkeypatch.setattr(gnn, "predict_mask", lambda logits: logits.argmax(1))      # (the mask kernel needs a GPU)
    for on in (True, False):
        monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", on)
        for loss in (fake(gnn.TverskyLoss, alpha=0.3, beta=0.7, gamma=0.75), fake(gnn.JaccardLoss)):
            calls.clear()
            t = SegmentationDOFA("dofa_base", pretrained=False, image_size=(8, 8), num_classes=5, max_samples=1, loss=loss)
            t.model = Model()
            t.training_step(batch, 0)
            with torch.no_grad():
                t.validation_step(batch, 0)
            assert calls == [on, on]


def test_overlap_options_struct_matches_the_header():
    """The ctypes mirror of gdl_overlap_options has the header's field order, and c_arg() fills it."""
    from gdlhip import _lib
    text = (Path(__file__).resolve().parents[1] / "include" / "gdlhip.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} gdl_overlap_options;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.strip().split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
    assert fields == ["kind", "has_ignore", "ignore_index", "smooth", "log_loss", "alpha", "beta", "gamma", "classes", "nclasses"]
    assert [f[0] for f in _lib.OverlapOptions._fields_] == fields
    kinds = {n: int(v) for n, v in re.findall(r"#define GDL_OVERLAP_(JACCARD|TVERSKY)\s+(\d+)", text)}
    assert kinds == {"JACCARD": _lib.OVERLAP_JACCARD, "TVERSKY": _lib.OVERLAP_TVERSKY}
    ptr, keep = ops.OverlapOptions("tversky", -1, 0.5, True, (1, 3), 0.25, 0.75, 2.0).c_arg()
    o = keep[0]
    assert (o.kind, o.has_ignore, o.ignore_index, o.smooth, o.log_loss, o.nclasses) == (_lib.OVERLAP_TVERSKY, 1, -1, 0.5, 1, 2)
    assert (o.alpha, o.beta, o.gamma) == (0.25, 0.75, 2.0)
    assert [o.classes[i] for i in range(2)] == [1, 3] and ptr
    o = ops.OverlapOptions("jaccard").c_arg()[1][0]
    assert (o.kind, o.has_ignore, o.nclasses) == (_lib.OVERLAP_JACCARD, 0, 0) and not o.classes
    # the existing public struct is unchanged
    assert [f[0] for f in _lib.DiceOptions._fields_] == ["has_ignore_index", "ignore_index", "smooth", "log_loss", "classes",
                                                         "num_classes"]


# ------------------------------------------------------------------------------------------------ restatement sanity
@pytest.mark.parametrize("kw", [dict(), dict(ignore_index=255), dict(log_loss=True), dict(classes=[1, 3])],
                         ids=["default", "ignore", "log_loss", "classes"])
def test_tversky_restatement_with_half_weights_is_dice(kw):
    """alpha = beta = 0.5, gamma = 1, smooth = 0: I / (I + (P - I)/2 + (Y - I)/2) = 2I / (P + Y)."""
    from test_hip_dice_options import dice_ref
    x, y = _inputs(1, ignore=kw.get("ignore_index"))
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    tv, score, ysum, _ = overlap_ref(a, y, "tversky", **kw)
    dc, dscore, dysum = dice_ref(b, y, **kw)
    assert abs(tv.item() - dc.item()) <= 1e-13 and torch.equal(ysum, dysum)
    assert (score - dscore).abs().max().item() <= 1e-13
    assert abs(overlap_ref(x, y, "dice", **kw)[0].item() - dc.item()) <= 1e-15
    tv.backward()
    dc.backward()
    assert (a.grad - b.grad).abs().max().item() <= 1e-14


def test_jaccard_restatement_is_d_over_two_minus_d_of_the_dice_score():
    x, y = _inputs(2)
    jl, jscore, ysum, _ = overlap_ref(x, y, "jaccard")
    _, d, _, _ = overlap_ref(x, y, "dice")
    assert (jscore - d / (2.0 - d)).abs().max().item() <= 1e-14
    want = ((1.0 - d / (2.0 - d)) * (ysum > 0)).mean()
    assert abs(jl.item() - want.item()) <= 1e-14
    # and Jaccard is Tversky with alpha = beta = 1: the form the kernels evaluate it in
    tl, tscore, _, _ = overlap_ref(x, y, "tversky", alpha=1.0, beta=1.0)
    assert abs(jl.item() - tl.item()) <= 1e-14 and (jscore - tscore).abs().max().item() <= 1e-14


def test_restatement_gradient_has_the_two_coefficient_shape():
    """dL/dp_ik = ca_k [y_i = k] + cb_k with the coefficients the issue derives (what dice_coeffs feeds the pixel kernels)."""
    x, y = _inputs(3)
    alpha, beta, gamma, smooth = 0.3, 0.7, 0.75, 1.0
    p = x.softmax(1).clone().requires_grad_(True)
    k = x.shape[1]
    hot = F.one_hot(y, k).permute(0, 3, 1, 2).double()
    inter, psum, ysum = (p * hot).sum((0, 2, 3)), p.sum((0, 2, 3)), hot.sum((0, 2, 3))
    num, den = inter + smooth, inter + alpha * (psum - inter) + beta * (ysum - inter) + smooth
    m = ((1 - num / den) * (ysum > 0)).mean()
    (m ** gamma).backward()
    with torch.no_grad():
        f = -(ysum > 0).double() / k * gamma * m ** (gamma - 1)
        ca = f * (den - num * (1 - alpha - beta)) / den ** 2
        cb = -f * num * alpha / den ** 2
        closed = ca[None, :, None, None] * hot + cb[None, :, None, None]
    assert (p.grad - closed).abs().max().item() <= 1e-15
