"""GPU tests of the inference tail: ``ops.normalize_range`` (the caller's sensor range), ``ops.upsample_probs`` (class probabilities
straight from a head's low-resolution map), ``gnn.predict_probs`` and the DOFA-backed ``SegmentationScriptModel`` end to end.

Bounds.  Reference against reference, the code under test never enters them (the convention of tests/test_hip_optimizers.py):
the yardstick is the reference's formula in f64 on the CPU, evaluated on the same f32 / integer inputs, and a case's bound is
4 x the largest deviation of torch's OWN f32 CPU evaluation of that formula from the f64 result, with a floor of one f32 ulp of
the largest output magnitude.  Every figure is printed before it is asserted (``pytest -s``).

Figures measured on an MI355X (DESIGN.md "The inference tail" has the table): normalize_range deviates from f64 by exactly what
torch's f32 CPU evaluation does in all 12 cases (2e-7 .. 1.4e-4 at outputs of 2 .. 1.2e3) and equals normalize_raw bit for bit on
the default range; upsample_probs stays within 0.7 .. 1.9 x torch's own f32 deviation (the closest to its bound: K = 1, 3x5 -> 12x20,
1.56e-7 against 3.28e-7), equals upsample_logits + class_probs bit for bit for K >= 2 and to 1.2e-7 for K = 1, |sum - 1| <= 3.5e-7.
"""

import functools
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
import oracle  # noqa: E402
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402
from geo_deep_learning.models.encoders.dofa_v2 import DOFAv2  # noqa: E402
from geo_deep_learning.models.segmentation.dofa import DOFASegmentationModel  # noqa: E402
from geo_deep_learning.tools.script_model import SegmentationScriptModel  # noqa: E402
from oracle import procedural_state_dict, synthetic_batch  # noqa: E402
from oracle.model import RGB_MEAN, RGB_STD  # noqa: E402

DEV = "cuda"


def _ulp(t: torch.Tensor) -> float:
    return float(np.spacing(np.float32(t.abs().max().item())))


def _bound(want64: torch.Tensor, own32: torch.Tensor) -> tuple[float, float]:
    """(bound, torch's own f32 deviation): 4 x own, at least one f32 ulp of the output magnitude."""
    own = (own32.double() - want64).abs().max().item()
    return max(4 * own, _ulp(want64)), own


# ------------------------------------------------------------------ normalize_range
RANGES = [(0, 255, 0.0, 1.0), (0, 65535, 0.0, 1.0), (-1000, 10000, -1.0, 1.0)]
DTYPES = {"uint8": (np.uint8, 0, 255), "uint16": (np.uint16, 0, 65535), "int16": (np.int16, -32768, 32767), "float32": (np.float32, -2000.0, 70000.0)}
MEAN = torch.tensor([0.485, 0.456, 0.406])
STD = torch.tensor([0.229, 0.224, 0.225])


@functools.lru_cache(maxsize=None)
def _raw_tile(kind: str) -> torch.Tensor:
    """[2, 3, 5, 7] (H*W = 35: groups of four straddle channels, two elements are left behind the last whole group) with the
    extreme representable values of the integer dtypes (the ends of the drawn interval for f32) in every channel."""
    npdt, lo, hi = DTYPES[kind]
    g = np.random.default_rng([11, len(kind)])
    if kind == "float32":
        a = g.uniform(lo, hi, (2, 3, 5, 7)).astype(npdt)
    else:
        a = g.integers(lo, hi + 1, (2, 3, 5, 7)).astype(npdt)
    a[:, :, 0, 0], a[:, :, 4, 6], a[:, :, 2, 3] = lo, hi, 0
    return torch.from_numpy(a)


def _formula(x: torch.Tensor, rng, mean: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    """utils/tensors.py:19-21 then :34, in the dtype of ``x`` (Python scalars meet the tensor as torch casts them)."""
    image_min, image_max, norm_min, norm_max = rng
    y = (norm_max - norm_min) * (x - image_min) / (image_max - image_min) + norm_min
    return (y - mean.to(x.dtype).view(1, -1, 1, 1)) / std.to(x.dtype).view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def _normalize_reference(kind: str, rng) -> tuple[torch.Tensor, float, float]:
    raw = _raw_tile(kind)
    want = _formula(raw.double(), rng, MEAN, STD)
    bound, own = _bound(want, _formula(raw.float(), rng, MEAN, STD))
    return want, bound, own


@pytest.mark.parametrize("rng", RANGES, ids=lambda r: f"{r[0]}..{r[1]}->{r[2]:g}..{r[3]:g}")
@pytest.mark.parametrize("kind", list(DTYPES))
def test_normalize_range_matches_the_f64_formula(kind, rng):
    want, bound, own = _normalize_reference(kind, rng)
    raw = _raw_tile(kind).to(DEV)
    got = ops.normalize_range(raw, MEAN.to(DEV), STD.to(DEV), *rng)
    assert got.dtype == torch.float32 and got.shape == raw.shape
    err = (got.cpu().double() - want).abs().max().item()
    print(f"normalize_range {kind} {rng}: kernel-f64 {err:.3e}  torch f32-f64 {own:.3e}  bound {bound:.3e}  |out| max {want.abs().max().item():.3e}")
    assert err <= bound
    if rng == RANGES[0]:
        base = ops.normalize_raw(raw, MEAN.to(DEV), STD.to(DEV))
        d = (got - base).abs().max().item()
        print(f"normalize_range {kind} default range vs normalize_raw: {d:.3e}")
        assert d <= bound


def test_normalize_range_unaligned_and_multi_block():
    """A view at an odd offset takes the one-element-per-thread kernel; 3 x 67 x 129 elements span several blocks of both."""
    g = np.random.default_rng(5)
    a = torch.from_numpy(g.integers(0, 65536, (1 + 2 * 3 * 67 * 129,)).astype(np.uint16))
    rng = RANGES[2]
    dev = a.to(DEV)
    for off in (0, 1):
        raw = dev[off:off + 2 * 3 * 67 * 129].view(2, 3, 67, 129)
        host = a[off:off + 2 * 3 * 67 * 129].view(2, 3, 67, 129)
        want = _formula(host.double(), rng, MEAN, STD)
        bound, own = _bound(want, _formula(host.float(), rng, MEAN, STD))
        err = (ops.normalize_range(raw, MEAN.to(DEV), STD.to(DEV), *rng).cpu().double() - want).abs().max().item()
        print(f"normalize_range offset {off}: kernel-f64 {err:.3e}  torch f32-f64 {own:.3e}  bound {bound:.3e}")
        assert err <= bound


def test_normalize_range_rejects_an_empty_range():
    raw = _raw_tile("uint8").to(DEV)
    with pytest.raises(ValueError, match="image_max == image_min"):
        ops.normalize_range(raw, MEAN.to(DEV), STD.to(DEV), 7, 7, 0.0, 1.0)
    from gdlhip import _lib
    out = torch.empty(raw.shape, device=DEV)
    status = _lib.load().gdl_normalize_range(raw.data_ptr(), 0, out.data_ptr(), 2, 3, 35, 7, 7, 0.0, 1.0, MEAN.to(DEV).data_ptr(),
                                             STD.to(DEV).data_ptr(), None)
    assert status == -1 and b"image_max == image_min" in _lib.load().gdl_last_error()


# ------------------------------------------------------------------ upsample_probs
# 3x5 -> 12x20 an integer factor on a non-square map, 7x7 -> 16x16 a non-integer factor, 8x8 -> 8x8 the identity; and, for the
# code's other paths: 3x5 -> 9x15 (Wo % 4 != 0: one pixel per thread, two blocks), 7x7 -> 64x52 (several blocks of the
# four-pixel kernel), 8x8 -> 5x6 (a downsample, which gdl_upsample_logits takes too)
SIZES = [((3, 5), (12, 20)), ((7, 7), (16, 16)), ((8, 8), (8, 8)), ((3, 5), (9, 15)), ((7, 7), (64, 52)), ((8, 8), (5, 6))]
CLASSES = [1, 2, 5, 16]


def _torch_probs(low: torch.Tensor, size) -> torch.Tensor:
    x = F.interpolate(low.permute(0, 3, 1, 2), size=tuple(size), mode="bilinear", align_corners=False)
    return x.softmax(dim=1) if x.shape[1] > 1 else x.sigmoid()


@functools.lru_cache(maxsize=None)
def _probs_case(k: int, lo, size):
    """Logits of magnitude up to +-30 (exp(30) * 16 overflows nothing, exp(60) would: a softmax without max-subtraction fails)."""
    g = torch.Generator().manual_seed(1000 * k + 10 * lo[0] + size[1])
    low = (torch.rand(2, lo[0], lo[1], k, generator=g) * 2 - 1) * 30
    low[0, 0, 0, :] = 30.0
    low[0, 0, 0, 0] = -30.0
    low[1, -1, -1, :] = -30.0
    low[1, -1, -1, -1] = 30.0
    want = _torch_probs(low.double(), size)
    bound, own = _bound(want, _torch_probs(low, size))
    return low, want, bound, own


@pytest.mark.parametrize("lo,size", SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("k", CLASSES)
def test_upsample_probs(k, lo, size):
    low, want, bound, own = _probs_case(k, lo, size)
    dlow = low.to(DEV)
    got = ops.upsample_probs(dlow, size)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, k, *size) and got.is_contiguous()
    two_pass = ops.class_probs(ops.upsample_logits(dlow, size))
    err = (got.cpu().double() - want).abs().max().item()
    err2 = (got - two_pass).abs().max().item()
    print(f"upsample_probs K={k} {lo}->{size}: kernel-f64 {err:.3e}  torch f32-f64 {own:.3e}  bound {bound:.3e}  vs upsample_logits+class_probs {err2:.3e}")
    assert torch.isfinite(got).all()
    assert err <= bound
    assert err2 <= bound
    if k > 1:
        top2 = want.topk(2, dim=1).values
        decided = ((top2[:, 0] - top2[:, 1]) > bound).to(DEV)
        assert torch.equal(got.argmax(1)[decided], two_pass.argmax(1)[decided])
        assert torch.equal(got.argmax(1)[decided].cpu(), want.argmax(1)[decided.cpu()])
        s = (got.double().sum(1) - 1).abs().max().item()
        print(f"upsample_probs K={k} {lo}->{size}: |sum - 1| max {s:.3e}")
        assert s <= 1e-6


def test_predict_probs_routes_on_the_device():
    """1..16 classes: the one-pass kernel's values; 17 classes and a bf16 map: materialise + class_probs; a tensor: class_probs."""
    low, want, bound, _ = _probs_case(5, (7, 7), (16, 16))
    dlow = low.to(DEV)
    assert torch.equal(gnn.predict_probs(gnn.LowresLogits(dlow, (16, 16))), ops.upsample_probs(dlow, (16, 16)))
    assert torch.equal(gnn.predict_probs(ops.upsample_logits(dlow, (16, 16))), ops.class_probs(ops.upsample_logits(dlow, (16, 16))))
    g = torch.Generator().manual_seed(17)
    low17 = (torch.rand(2, 7, 7, 17, generator=g) * 2 - 1) * 30
    got = gnn.predict_probs(gnn.LowresLogits(low17.to(DEV), (16, 16)))
    mat = ops.class_probs(gnn.LowresLogits(low17.to(DEV), (16, 16)).materialise())
    want17 = _torch_probs(low17.double(), (16, 16))
    bound17, own17 = _bound(want17, _torch_probs(low17, (16, 16)))
    err = (got.cpu().double() - want17).abs().max().item()
    print(f"predict_probs K=17: kernel-f64 {err:.3e}  torch f32-f64 {own17:.3e}  bound {bound17:.3e}")
    assert tuple(got.shape) == (2, 17, 16, 16) and torch.equal(got, mat) and err <= bound17
    assert (got.double().sum(1) - 1).abs().max().item() <= 1e-6
    with pytest.raises(ValueError, match="1..16 classes"):
        ops.upsample_probs(low17.to(DEV), (16, 16))
    bf = gnn.predict_probs(gnn.LowresLogits(dlow.bfloat16(), (16, 16)))
    assert torch.equal(bf, ops.class_probs(ops.upsample_logits(dlow.bfloat16().float(), (16, 16))))
    assert not gnn.predict_probs(gnn.LowresLogits(dlow.requires_grad_(), (16, 16))).requires_grad


# ------------------------------------------------------------------ SegmentationScriptModel, DOFA, end to end
class _HidesLowres(torch.nn.Module):
    """The model behind a forward without ``lowres_logits``: the wrapper then resizes the logits and runs class_probs over them."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x, wavelengths):
        return self.inner(x, wavelengths)


@pytest.fixture(scope="module", params=[5, 1], ids=["softmax5", "sigmoid1"])
def dofa(request, golden_dir):
    """The smallest DOFA configuration of tests/test_hip_model.py (``tiny``), 3 bands, batch 2, procedural weights."""
    meta = json.loads(str(np.load(golden_dir / "dofa_tiny.npz")["meta"]))
    nc, img = request.param, meta["img"]
    ref = oracle.DOFASegmentationModel("dofa_tiny_test", (img, img), num_classes=nc, _encoder_kwargs=meta["tiny"], freeze_layers=["encoder"])
    sd = procedural_state_dict(ref, meta["seed"])
    model = DOFASegmentationModel(DOFAv2(img_size=img, pretrained=False, **meta["tiny"]), (img, img), num_classes=nc, pretrained=False,
                                  freeze_layers=["encoder"])
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    batch = synthetic_batch(2, 3, img, max(nc, 2), meta["seed"])
    kw = dict(wavelengths=batch["wavelengths"], device=torch.device(DEV), num_classes=nc, input_shape=(1, 3, img, img), mean=RGB_MEAN, std=RGB_STD)
    return nc, img, model, batch, kw


def test_script_model_lowres_route_equals_the_resized_route(dofa, monkeypatch):
    nc, img, model, batch, kw = dofa
    on, off = SegmentationScriptModel(model, **kw), SegmentationScriptModel(_HidesLowres(model), **kw)
    assert on.lowres and not off.lowres
    want = off(batch["image_u8"])

    def no_full_logits(*a, **k):
        raise AssertionError("the low-resolution route must not write the [B, K, H, W] logits")

    monkeypatch.setattr(ops, "upsample_logits", no_full_logits)
    got = on(batch["image_u8"])
    monkeypatch.undo()
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, nc, img, img) and not got.requires_grad
    with torch.no_grad():
        x = ops.normalize_raw(batch["image_u8"].to(DEV), on.mean, on.std)
        low = model(x, batch["wavelengths"], lowres_logits=True).out.low.cpu()
    ref64 = _torch_probs(low.double(), (img, img))
    bound, own = _bound(ref64, _torch_probs(low, (img, img)))
    d = (got - want).abs().max().item()
    err = (got.cpu().double() - ref64).abs().max().item()
    print(f"script model K={nc}: low-resolution route vs resized route {d:.3e}  vs f64 of the head's map {err:.3e}  torch f32-f64 {own:.3e}  bound {bound:.3e}")
    assert d <= bound and err <= bound
    if nc > 1:
        assert (got.double().sum(1) - 1).abs().max().item() <= 1e-6


def test_script_model_from_logits_false_returns_the_resized_logits(dofa):
    nc, img, model, batch, kw = dofa
    wrap = SegmentationScriptModel(model, from_logits=False, **kw)
    got = wrap(batch["image_u8"])
    with torch.no_grad():
        want = model(ops.normalize_raw(batch["image_u8"].to(DEV), wrap.mean, wrap.std), batch["wavelengths"]).out
    assert tuple(got.shape) == (2, nc, img, img) and torch.equal(got, want)


def test_script_model_uint16_tile_matches_its_uint8_counterpart(dofa):
    """u16 = 257 * u8 (65535 / 255 = 257) with image_max=65535 is the same tile.  The bound is what torch's own f32 evaluation of
    the two normalisations differs by, propagated through the f32 model: the two f32 inputs are formed on the CPU, fed to the
    model, and the largest difference of the probabilities is measured (x 4, floor one ulp) -- no number fixed in advance.
    Measured: 0 (x / 255 and 257 x / 65535 are the same rational, correctly rounded once in either form), so the floor holds."""
    nc, img, model, batch, kw = dofa
    u8 = batch["image_u8"]
    u16 = torch.from_numpy(u8.numpy().astype(np.uint16) * np.uint16(257))
    p8 = SegmentationScriptModel(model, **kw)(u8)
    p16 = SegmentationScriptModel(model, image_max=65535, **kw)(u16)
    mean, std = torch.tensor(RGB_MEAN), torch.tensor(RGB_STD)
    xa, xb = _formula(u8.float(), (0, 255, 0.0, 1.0), mean, std), _formula(u16.float(), (0, 65535, 0.0, 1.0), mean, std)
    with torch.no_grad():
        pa = gnn.predict_probs(model(xa.to(DEV), batch["wavelengths"], lowres_logits=True).out)
        pb = gnn.predict_probs(model(xb.to(DEV), batch["wavelengths"], lowres_logits=True).out)
    propagated = (pa - pb).abs().max().item()
    bound = max(4 * propagated, _ulp(pa))
    d = (p16 - p8).abs().max().item()
    print(f"script model K={nc}: uint16 vs uint8 tile {d:.3e}  torch f32 inputs propagated {propagated:.3e} (inputs differ by "
          f"{(xa - xb).abs().max().item():.3e})  bound {bound:.3e}")
    assert d <= bound
