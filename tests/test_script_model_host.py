"""The inference wrappers' input range and probability route, the parts that need no GPU: ``ScriptModel`` accepts any
``image_min`` / ``image_max`` / ``norm_min`` / ``norm_max`` (an empty range is a ValueError), the reference defaults keep the
``/255`` kernel and every other range takes ``ops.normalize_range``, a model whose ``forward`` takes ``lowres_logits`` is asked for
its heads' own maps, ``gnn.predict_probs`` routes them to the one-pass kernel or materialises them, and the two new C symbols are
declared in include/gdlhip.h as their ctypes signatures say."""

import re
from pathlib import Path

import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import _lib  # noqa: E402
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402
from geo_deep_learning.models.heads.segmentation_head import SegmentationOutput  # noqa: E402
from geo_deep_learning.tools.script_model import ScriptModel, SegmentationScriptModel  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CPU = torch.device("cpu")


class Plain(torch.nn.Module):
    """A model with a full-resolution head (UNet++): no ``lowres_logits`` argument."""

    def __init__(self, k=3):
        super().__init__()
        self.k, self.calls = k, []

    def forward(self, x):
        self.calls.append({})
        return torch.zeros(x.shape[0], self.k, *x.shape[2:])


class Lowres(torch.nn.Module):
    """A model shaped like DOFASegmentationModel.forward: (out, aux), the heads' maps on request."""

    def __init__(self, k=3):
        super().__init__()
        self.k, self.calls = k, []

    def forward(self, x, wavelengths, drop_masks=None, aux_drop_mask=None, lowres_logits=False):
        self.calls.append({"wavelengths": wavelengths, "lowres_logits": lowres_logits})
        b, (h, w) = x.shape[0], x.shape[2:]
        if lowres_logits:
            out = gnn.LowresLogits(torch.zeros(b, h // 4, w // 4, self.k), (h, w))
            return SegmentationOutput(out=out, aux="aux")
        return SegmentationOutput(out=torch.zeros(b, self.k, h, w), aux="aux")


def test_any_range_constructs():
    """Fails before this feature: anything but 0, 255, 0.0, 1.0 raised NotImplementedError."""
    m = ScriptModel(Plain(), device=CPU, num_classes=3, input_shape=(1, 3, 8, 8), image_max=65535)
    assert (m.image_min, m.image_max, m.norm_min, m.norm_max) == (0, 65535, 0.0, 1.0)
    m = SegmentationScriptModel(Lowres(), wavelengths=torch.ones(3), device=CPU, image_min=-1000, image_max=10000, norm_min=-1, norm_max=1)
    assert (m.image_min, m.image_max, m.norm_min, m.norm_max) == (-1000, 10000, -1.0, 1.0)


@pytest.mark.parametrize("lo,hi", [(0, 0), (255, 255), (-7, -7), (3.2, 3.9)], ids=str)
def test_empty_range_is_a_value_error(lo, hi):
    """(the reference takes ``int(image_min)`` / ``int(image_max)``: 3.2 and 3.9 are the same bound)"""
    with pytest.raises(ValueError, match="image_max == image_min"):
        ScriptModel(Plain(), device=CPU, image_min=lo, image_max=hi)
    with pytest.raises(ValueError, match="image_max == image_min"):
        ops.normalize_range(torch.zeros(1, 3, 2, 2), torch.zeros(3), torch.ones(3), int(lo), int(hi), 0.0, 1.0)


def _record_ops(monkeypatch):
    seen = []
    monkeypatch.setattr(ops, "normalize_raw", lambda x, mean, std: seen.append(("raw", x.dtype)) or x.float())
    monkeypatch.setattr(ops, "normalize_range", lambda x, mean, std, *rng: seen.append(("range", x.dtype, rng)) or x.float())
    monkeypatch.setattr(ops, "class_probs", lambda t: seen.append(("class_probs", tuple(t.shape))) or t)
    monkeypatch.setattr(ops, "upsample_probs", lambda low, size: seen.append(("upsample_probs", tuple(low.shape), tuple(size))) or "probs")
    return seen


def test_defaults_keep_normalize_raw_and_any_other_range_takes_normalize_range(monkeypatch):
    seen = _record_ops(monkeypatch)
    x = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    ScriptModel(Plain(), device=CPU, num_classes=3, input_shape=(1, 3, 8, 8))(x)
    ScriptModel(Plain(), device=CPU, num_classes=3, input_shape=(1, 3, 8, 8), image_min=0.0, image_max=255.0, norm_min=0, norm_max=1)(x)
    assert [s[0] for s in seen] == ["raw", "class_probs"] * 2
    for rng in ((0, 65535, 0.0, 1.0), (-1000, 10000, -1.0, 1.0), (0, 255, 0.0, 2.0), (1, 255, 0.0, 1.0), (0, 255, 0.5, 1.0)):
        seen.clear()
        ScriptModel(Plain(), device=CPU, num_classes=3, input_shape=(1, 3, 8, 8), image_min=rng[0], image_max=rng[1], norm_min=rng[2],
                    norm_max=rng[3])(x.to(torch.uint16))
        assert seen == [("range", torch.uint16, rng), ("class_probs", (2, 3, 8, 8))]
    seen.clear()
    ScriptModel(Plain(), device=CPU, image_max=65535)(torch.zeros(1, 3, 8, 8, dtype=torch.float64))     # anything else goes in as f32
    assert seen[0] == ("range", torch.float32, (0, 65535, 0.0, 1.0))


def test_a_model_with_lowres_logits_is_asked_for_its_maps(monkeypatch):
    seen = _record_ops(monkeypatch)
    wv = torch.tensor([0.6, 0.5, 0.4])
    model = Lowres()
    wrap = SegmentationScriptModel(model, wavelengths=wv, device=CPU, num_classes=3, input_shape=(1, 3, 8, 8))
    assert wrap(torch.zeros(2, 3, 8, 8, dtype=torch.uint8)) == "probs"
    assert len(model.calls) == 1 and model.calls[0]["wavelengths"] is wv and model.calls[0]["lowres_logits"] is True
    assert seen == [("raw", torch.uint8), ("upsample_probs", (2, 2, 2, 3), (8, 8))], "the main output only, never materialised"
    # from_logits=False: the resized logits, as the reference returns them
    monkeypatch.setattr(gnn.LowresLogits, "materialise", lambda self: ("materialised", tuple(self.low.shape), tuple(self.size)))
    seen.clear()
    wrap = SegmentationScriptModel(model, wavelengths=wv, device=CPU, num_classes=3, input_shape=(1, 3, 8, 8), from_logits=False)
    assert wrap(torch.zeros(2, 3, 8, 8, dtype=torch.uint8)) == ("materialised", (2, 2, 2, 3), (8, 8))
    assert seen == [("raw", torch.uint8)]


def test_a_model_without_lowres_logits_keeps_its_path(monkeypatch):
    seen = _record_ops(monkeypatch)
    model = Plain()
    wrap = SegmentationScriptModel(model, device=CPU, num_classes=3, input_shape=(1, 3, 8, 8))
    out = wrap(torch.zeros(2, 3, 8, 8, dtype=torch.uint8))
    assert model.calls == [{}] and tuple(out.shape) == (2, 3, 8, 8)
    assert seen == [("raw", torch.uint8), ("class_probs", (2, 3, 8, 8))]

    class Hidden(torch.nn.Module):           # a wrapper whose forward hides the argument disables the route
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x, wavelengths):
            return self.inner(x, wavelengths)

    seen.clear()
    inner = Lowres()
    wrap = SegmentationScriptModel(Hidden(inner), wavelengths=torch.ones(3), device=CPU, num_classes=3, input_shape=(1, 3, 8, 8))
    wrap(torch.zeros(2, 3, 8, 8, dtype=torch.uint8))
    assert [c["lowres_logits"] for c in inner.calls] == [False]
    assert seen == [("raw", torch.uint8), ("class_probs", (2, 3, 8, 8))]


def test_predict_probs_routing(monkeypatch):
    taken = []
    monkeypatch.setattr(ops, "upsample_probs", lambda low, size: taken.append(("upsample_probs", low.shape[3], size)) or "fused")
    monkeypatch.setattr(ops, "class_probs", lambda t: taken.append(("class_probs", tuple(t.shape), t.dtype, t.is_contiguous())) or "probs")
    monkeypatch.setattr(gnn.LowresLogits, "materialise", lambda self: taken.append(("materialise", self.low.shape[3])) or torch.zeros(2, self.low.shape[3], 8, 8))
    for k in (1, 2, 16):
        taken.clear()
        assert gnn.predict_probs(gnn.LowresLogits(torch.zeros(2, 4, 4, k), [8, 8])) == "fused"
        assert taken == [("upsample_probs", k, (8, 8))]
    for low in (torch.zeros(2, 4, 4, 17), torch.zeros(2, 4, 4, 5, dtype=torch.bfloat16)):
        taken.clear()
        assert gnn.predict_probs(gnn.LowresLogits(low, (8, 8))) == "probs"
        assert taken == [("materialise", low.shape[3]), ("class_probs", (2, low.shape[3], 8, 8), torch.float32, True)]
    taken.clear()
    assert gnn.predict_probs(torch.zeros(2, 5, 8, 8, dtype=torch.bfloat16).transpose(2, 3)) == "probs"
    assert taken == [("class_probs", (2, 5, 8, 8), torch.float32, True)]
    grad = []
    monkeypatch.setattr(ops, "class_probs", lambda t: grad.append(torch.is_grad_enabled()) or "probs")
    gnn.predict_probs(torch.zeros(2, 5, 8, 8, requires_grad=True))       # inference only: evaluated under no_grad
    assert grad == [False] and torch.is_grad_enabled()


def test_op_argument_errors_come_before_the_device():
    mean, std = torch.zeros(3), torch.ones(3)
    with pytest.raises(ValueError, match="device tensors"):
        ops.normalize_range(torch.zeros(1, 3, 2, 2), mean, std, 0, 65535, 0.0, 1.0)
    with pytest.raises(ValueError, match="contiguous NCHW"):
        ops.normalize_range(torch.zeros(1, 3, 2, 2, dtype=torch.int32), mean, std, 0, 65535, 0.0, 1.0)
    with pytest.raises(ValueError, match="device tensors"):
        ops.upsample_probs(torch.zeros(1, 2, 2, 3), (4, 4))


def test_signatures_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gdlhip.h").read_text(), flags=re.S)
    kinds_of = {"int64_t": _lib.c_l, "float": _lib.c_f, "double": _lib.C.c_double, "int": _lib.c_i}
    for name in ("gdl_normalize_range", "gdl_upsample_probs"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/gdlhip.h"
        res, args = _lib.SIGNATURES[name]
        kinds = []
        for decl in m.group(1).split(","):
            decl = decl.strip()
            if "*" in decl or decl.startswith("gdl_stream_t"):
                kinds.append(_lib.c_p)
            else:
                kinds.append(kinds_of[decl.split()[0]])
        assert res is _lib.c_i and kinds == list(args), name
