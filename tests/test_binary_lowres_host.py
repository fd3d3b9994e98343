"""One-class (binary) segmentation from the heads' low-resolution maps, the parts that need no GPU: the ``reads_lowres``
predicate with and without ``num_classes``, the ctypes signatures against include/gdlhip.h, the argument errors the op wrappers
raise before anything touches a device, the routing of the options to the C symbols, and the task hooks (``_predict`` on a CPU
tensor keeps the reference's expression; a one-class DOFA task asks the model for its low-resolution maps)."""

import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import _lib  # noqa: E402
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
NEW = ["gdl_sigmoid_threshold", "gdl_upsample_threshold", "gdl_binary_lowres_bwd_workspace",
       "gdl_dice_binary_loss_lowres_fwd", "gdl_dice_binary_loss_lowres_bwd", "gdl_dice_binary_loss_lowres_opt_fwd",
       "gdl_dice_binary_loss_lowres_opt_bwd", "gdl_overlap_binary_loss_lowres_fwd", "gdl_overlap_binary_loss_lowres_bwd",
       "gdl_focal_binary_lowres_fwd", "gdl_focal_binary_lowres_bwd"]


def _binary_losses():
    return [gnn.DiceLoss(mode="binary"), gnn.DiceLoss(mode="binary", smooth=1.0, log_loss=True, ignore_index=255),
            gnn.JaccardLoss(mode="binary"), gnn.TverskyLoss(mode="binary", alpha=0.3, beta=0.7, gamma=0.75, ignore_index=-1),
            gnn.FocalLoss("binary", alpha=0.25)]


def test_reads_lowres_with_and_without_num_classes():
    for loss in _binary_losses():
        assert gnn.reads_lowres(loss) is False, "the default is today's value"
        assert gnn.reads_lowres(loss, None) is False
        assert gnn.reads_lowres(loss, 1) is True
        assert gnn.reads_lowres(loss, num_classes=5) is False, "a binary loss on a K-class head has no low-resolution form"
    for loss in (gnn.DiceLoss(), gnn.JaccardLoss(), gnn.TverskyLoss(), gnn.FocalLoss("multiclass"), gnn.SoftCrossEntropyLoss(smooth_factor=0.1)):
        assert gnn.reads_lowres(loss) and gnn.reads_lowres(loss, 1) and gnn.reads_lowres(loss, 5)
    for loss in (gnn.LovaszLoss("binary"), gnn.LovaszLoss("multiclass"), torch.nn.CrossEntropyLoss()):
        assert not gnn.reads_lowres(loss) and not gnn.reads_lowres(loss, 1)


def test_signatures_match_the_header():
    """Every new symbol is declared in include/gdlhip.h with as many parameters, and the same int / int64 / float / pointer kinds, as
    its ctypes signature."""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gdlhip.h").read_text(), flags=re.S)
    for name in NEW:
        m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/gdlhip.h"
        res, args = _lib.SIGNATURES[name]
        assert res is (_lib.c_l if m.group(1) == "int64_t" else _lib.c_i)
        kinds = []
        for decl in m.group(2).split(","):
            decl = decl.strip()
            if "*" in decl or decl.startswith("gdl_stream_t"):
                kinds.append(_lib.c_p)
            elif decl.startswith("int64_t"):
                kinds.append(_lib.c_l)
            elif decl.startswith("float"):
                kinds.append(_lib.c_f)
            else:
                assert decl.startswith("int "), (name, decl)
                kinds.append(_lib.c_i)
        assert kinds == list(args), name


ROUTES = [(None, "gdl_dice_{}_{}"), (ops.DiceOptions(255), "gdl_dice_{}_opt_{}"), (ops.OverlapOptions("tversky", 255), "gdl_overlap_{}_{}")]


@pytest.mark.parametrize("options,pattern", ROUTES, ids=["plain", "dice-options", "overlap-options"])
def test_ops_route_options_to_the_entry_point_and_argument_positions(monkeypatch, options, pattern):
    """As tests/test_overlap_loss_host.py holds the existing stems: ``options`` picks the C symbol, the option pointer follows
    ``eps``, ``eps`` / ``grad_scale`` land on the float positions, the backward's ``form`` is the last int.  No library is loaded."""
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
    low, y, sums, up = torch.zeros(1, 2, 2, 1), torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(3), torch.ones(())
    for way, run in (("fwd", lambda: ops.dice_binary_lowres_fwd(low, y, (4, 4), EPS, options=options)),
                     ("bwd", lambda: ops.dice_binary_lowres_bwd(low, y, (4, 4), sums, up, GS, EPS, options=options, form="tile"))):
        calls.clear()
        run()
        want = pattern.format("binary_loss_lowres", way)
        assert [c[0] for c in calls] == [want]
        args, types = calls[0][1], _lib.SIGNATURES[want][1]
        assert len(args) == len(types) and args[-1] == 7
        floats = [i for i, t in enumerate(types) if t is C.c_float]
        assert args[floats[0]] == EPS and (way == "fwd" or args[floats[1]] == GS)
        assert args[2:7] == (1, 2, 2, 4, 4)
        if options is not None:
            assert isinstance(args[floats[0] + 1], int) and args[floats[0] + 1] != 0
        if way == "bwd":
            assert types[-2] is C.c_int and args[-2] == _lib.FOCAL_TILE


def test_argument_errors_are_raised_before_the_device_is_touched():
    """K != 1, a downsample and a factor above 64 are ValueErrors that name the fault (CPU tensors: the shape test comes first);
    a well-shaped CPU tensor is refused as every gdlhip op refuses it."""
    y = torch.zeros(1, 8, 8, dtype=torch.int64)
    sums, norm, up = torch.zeros(3), torch.ones(1), torch.ones(())

    def calls(low, size, tgt):
        return [lambda: ops.dice_binary_lowres_fwd(low, tgt, size), lambda: ops.dice_binary_lowres_bwd(low, tgt, size, sums, up),
                lambda: ops.focal_binary_lowres_fwd(low, tgt, size), lambda: ops.focal_binary_lowres_bwd(low, tgt, size, norm, up),
                lambda: ops.upsample_threshold(low, size)]

    for call in calls(torch.zeros(1, 4, 4, 2), (8, 8), y):
        with pytest.raises(ValueError, match=r"one-class .*\[B, h, w, 1\]"):
            call()
    for call in calls(torch.zeros(1, 4, 4), (8, 8), y):
        with pytest.raises(ValueError, match="one-class"):
            call()
    for low, size in ((torch.zeros(1, 12, 4, 1), (8, 8)), (torch.zeros(1, 4, 12, 1), (8, 8))):
        for call in calls(low, size, y):
            with pytest.raises(ValueError, match="an upsample is expected"):
                call()
    for low, size in ((torch.zeros(1, 1, 4, 1), (65, 8)), (torch.zeros(1, 4, 1, 1), (8, 65))):
        for call in calls(low, size, torch.zeros(1, *size, dtype=torch.int64)):
            with pytest.raises(ValueError, match="factors above 64"):
                call()
    for call in calls(torch.zeros(1, 1, 1, 1), (64, 64), torch.zeros(1, 64, 64, dtype=torch.int64)):      # factor 64 itself is a legal shape
        with pytest.raises(ValueError, match="device tensors"):
            call()
    with pytest.raises(ValueError, match="device tensors"):
        ops.sigmoid_threshold(torch.zeros(1, 1, 4, 4))
    with pytest.raises(ValueError, match=r"\[B, h, w, 1\]"):
        gnn.predict_binary_mask(gnn.LowresLogits(torch.zeros(1, 4, 4, 3), (8, 8)))
    with pytest.raises(ValueError, match=r"\[B, 1, H, W\]"):
        gnn.predict_binary_mask(torch.zeros(1, 3, 8, 8))


def test_losses_materialise_what_the_binary_kernels_do_not_take(monkeypatch):
    """The routing of _DiceFamily.forward / FocalLoss.forward: a one-class f32 map within the shape limits goes to the
    low-resolution ops, everything else (K != 1, a downsample, the switch off, a target at another size) is materialised."""
    taken = []
    monkeypatch.setattr(ops, "dice_binary_lowres_fwd", lambda *a, **k: taken.append("dice") or (torch.zeros(()), torch.zeros(3)))
    monkeypatch.setattr(ops, "focal_binary_lowres_fwd", lambda *a, **k: taken.append("focal") or (torch.zeros(()), torch.zeros(1)))

    class Materialised(Exception):
        pass

    def boom(self):
        raise Materialised

    monkeypatch.setattr(gnn.LowresLogits, "materialise", boom)
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    for crit, tag in ((gnn.DiceLoss(mode="binary"), "dice"), (gnn.TverskyLoss(mode="binary"), "dice"), (gnn.FocalLoss("binary"), "focal")):
        monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", True)
        taken.clear()
        crit(gnn.LowresLogits(torch.zeros(2, 4, 4, 1), (8, 8)), y)
        crit(gnn.LowresLogits(torch.zeros(2, 4, 4, 1), (8, 8)), y[:, None])      # an un-squeezed [B,1,H,W] mask
        assert taken == [tag, tag]
        for low, size, tgt in ((torch.zeros(2, 4, 4, 2), (8, 8), y), (torch.zeros(2, 16, 16, 1), (8, 8), y),
                               (torch.zeros(2, 4, 4, 1), (16, 16), y), (torch.zeros(2, 4, 4, 1, dtype=torch.bfloat16), (8, 8), y)):
            with pytest.raises(Materialised):
                crit(gnn.LowresLogits(low, size), tgt)
        # a factor above the measured range of the low-resolution kernels (ops.BINARY_LOWRES_MAX_FACTOR): the resized logits
        big = ops.BINARY_LOWRES_MAX_FACTOR * 2 + 1
        assert ops.dice_lowres_ok(torch.zeros(1, 2, 2, 1), (2 * big, 2 * big)) and not ops.binary_lowres_pays(torch.zeros(1, 2, 2, 1), (2 * big, 2 * big))
        edge = 2 * ops.BINARY_LOWRES_MAX_FACTOR
        assert ops.binary_lowres_pays(torch.zeros(1, 2, 2, 1), (edge, edge)) and not ops.binary_lowres_pays(torch.zeros(1, 2, 2, 2), (edge, edge))
        with pytest.raises(Materialised):
            crit(gnn.LowresLogits(torch.zeros(2, 2, 2, 1), (2 * big, 2 * big)), torch.zeros(2, 2 * big, 2 * big, dtype=torch.int64))
        monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", False)
        with pytest.raises(Materialised):
            crit(gnn.LowresLogits(torch.zeros(2, 4, 4, 1), (8, 8)), y)
        assert taken == [tag, tag]


def _hooks(num_classes, threshold=0.5):
    from geo_deep_learning.tasks_with_models._common import SegmentationTaskHooks
    h = SegmentationTaskHooks()
    h.num_classes, h.threshold = num_classes, threshold
    return h


def test_predict_on_a_cpu_tensor_is_unchanged(monkeypatch):
    def never(*a, **kw):
        raise AssertionError("the mask kernel must not be asked for a CPU tensor")

    monkeypatch.setattr(gnn, "predict_binary_mask", never)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 1, 9, 7, generator=g) * 2
    x[0, 0, 0, :3] = torch.tensor([0.0, 1e-8, -1e-8])
    for th in (0.5, 0.3):
        got = _hooks(1, th)._predict(x)
        assert got.dtype == torch.int64 and got.shape == (2, 9, 7)
        assert torch.equal(got, (x.sigmoid().squeeze(1) > th).long())
    assert _hooks(1)._predict(x)[0, 0, :3].tolist() == [0, 0, 0], "sigmoid(0) > 0.5 is False, and so is sigmoid(1e-8) in f32"


def test_predict_hands_device_and_low_resolution_logits_to_the_mask_kernel(monkeypatch):
    seen = []
    monkeypatch.setattr(gnn, "predict_binary_mask", lambda logits, th: seen.append((logits, th)) or "mask")
    low = gnn.LowresLogits(torch.zeros(1, 4, 4, 1), (8, 8))
    assert _hooks(1, 0.3)._predict(low) == "mask" and seen == [(low, 0.3)]

    class OnDevice:
        is_cuda = True

    dev = OnDevice()
    assert _hooks(1)._predict(dev) == "mask" and seen[-1] == (dev, 0.5)


def test_one_class_dofa_task_asks_for_low_resolution_logits(monkeypatch):
    """SegmentationDOFA with ``num_classes: 1`` and a binary gdlhip loss: training and validation hand the loss and the mask
    kernel the heads' own maps; with GDL_LOWRES_DICE=0, or a binary loss on a K-class head, the resized logits as before."""
    from tasks_with_models.segmentation_dofa import SegmentationDOFA
    calls, masks = [], []

    class Model(torch.nn.Module):
        def __init__(self, k):
            super().__init__()
            self.k = k

        def forward(self, x, wv, lowres_logits=False):
            calls.append(bool(lowres_logits))
            out = torch.zeros(x.shape[0], self.k, 8, 8, requires_grad=True)
            if lowres_logits:
                out = gnn.LowresLogits(torch.zeros(x.shape[0], 4, 4, self.k, requires_grad=True), (8, 8))
            return SimpleNamespace(out=out, aux=out)

    def fake(cls, *a, **kw):
        fwd = lambda self, y_pred, y_true: (y_pred.low if isinstance(y_pred, gnn.LowresLogits) else y_pred).sum() * 0.0  # noqa: E731
        return type("Fake" + cls.__name__, (cls,), {"forward": fwd})(*a, **kw)

    def task_with(loss, k):
        t = SegmentationDOFA("dofa_base", pretrained=False, image_size=(8, 8), num_classes=k, max_samples=1, loss=loss)
        t.model = Model(k)
        return t

    batch = {"image": torch.zeros(2, 3, 8, 8), "mask": torch.zeros(2, 1, 8, 8, dtype=torch.int64), "wavelengths": torch.tensor([0.6, 0.5, 0.4])}
    monkeypatch.setattr(gnn, "predict_binary_mask", lambda logits, th=0.5: masks.append(logits) or torch.zeros(2, 8, 8, dtype=torch.int64))
    monkeypatch.setattr(gnn, "predict_mask", lambda logits: logits.argmax(1))
    for on in (True, False):
        monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", on)
        for loss in (fake(gnn.DiceLoss, mode="binary"), fake(gnn.TverskyLoss, mode="binary"), fake(gnn.FocalLoss, "binary")):
            calls.clear(), masks.clear()
            t = task_with(loss, 1)
            t.training_step(batch, 0)
            with torch.no_grad():
                t.validation_step(batch, 0)
            assert calls == [on, on]
            # (on a host tensor the resized logits keep the reference's expression; the low-resolution map goes to the mask kernel)
            assert [isinstance(m, gnn.LowresLogits) for m in masks] == ([True] if on else [])
    monkeypatch.setattr(gnn, "FUSE_LOWRES_DICE", True)
    calls.clear()
    t = task_with(fake(gnn.DiceLoss, mode="binary"), 5)
    t.training_step(batch, 0)
    with torch.no_grad():
        t.validation_step(batch, 0)
    assert calls == [False, False]
