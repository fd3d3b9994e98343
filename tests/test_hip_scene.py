"""GPU tests of whole-scene inference: ``ops.scene_cut`` / ``scene_blend`` / ``scene_blend_lowres`` / ``scene_finish``
(include/gdlhip_scene.h) and ``SceneInference`` over the DOFA-backed ``SegmentationScriptModel``.

Three kinds of check.  Bit for bit against the kernels the scene kernels share their expressions with (``normalize_range``,
``upsample_probs``) and between batchings of one tile list.  Exactly against torch where the result is a decision (the mask).  And
against f64 with the rule of tests/test_hip_inference_tail.py: the yardstick is a torch restatement in f64 on the CPU, a case's
bound is 4 x the largest deviation of the SAME restatement evaluated in f32 on the CPU from it, with a floor of one f32 ulp of the
largest output magnitude; the code under test never enters a bound, every figure is printed before it is asserted (``pytest -s``)
and no pixel is excluded.

Figures measured on an MI355X: the blend stays within 0.6 .. 1.0 x torch's own f32 deviation in all 16 f64 cases (the closest to
its bound: K = 1, 37 x 53, 2.1e-7 against 8.4e-7), the labelled probabilities deviate by exactly what torch's f32 quotient does,
SceneInference's canvas by 1.7e-7 .. 2.8e-7 against bounds of 8.2e-7 .. 1.4e-6, and its two routes agree to the bit."""

import functools
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
import oracle  # noqa: E402
from gdlhip import ops  # noqa: E402
from gdlhip import scene as gscene  # noqa: E402
from geo_deep_learning.models.encoders.dofa_v2 import DOFAv2  # noqa: E402
from geo_deep_learning.models.segmentation.dofa import DOFASegmentationModel  # noqa: E402
from geo_deep_learning.tools.scene_inference import SceneInference  # noqa: E402
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


def _origins(pairs) -> torch.Tensor:
    return torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(DEV)


# ------------------------------------------------------------------ 1. cut
RANGES = [(0, 255, 0.0, 1.0), (0, 65535, 0.0, 1.0), (-1000, 10000, -1.0, 1.0)]      # those of tests/test_hip_inference_tail.py
DTYPES = {"uint8": (np.uint8, 0, 255), "uint16": (np.uint16, 0, 65535), "int16": (np.int16, -32768, 32767), "float32": (np.float32, -2000.0, 70000.0)}
MEAN = torch.tensor([0.485, 0.456, 0.406])
STD = torch.tensor([0.229, 0.224, 0.225])
CUT_ORIGINS = [(0, 0), (21, 37), (-3, -5), (30, 45)]      # inside, touching the far corner, overhanging before, overhanging after


@functools.lru_cache(maxsize=None)
def _raster(kind: str) -> np.ndarray:
    """[3, 37, 53] with the extreme values of the dtype in every channel."""
    npdt, lo, hi = DTYPES[kind]
    g = np.random.default_rng([23, len(kind)])
    a = g.uniform(lo, hi, (3, 37, 53)).astype(npdt) if kind == "float32" else g.integers(lo, hi + 1, (3, 37, 53)).astype(npdt)
    a[:, 0, 0], a[:, 36, 52], a[:, 20, 30] = lo, hi, 0
    return a


@pytest.mark.parametrize("tile", [(16, 16), (5, 7)], ids=["16x16", "5x7"])      # 16-byte stores; one value per thread
@pytest.mark.parametrize("fill", [0, 7])
@pytest.mark.parametrize("rng", RANGES, ids=lambda r: f"{r[0]}..{r[1]}->{r[2]:g}..{r[3]:g}")
@pytest.mark.parametrize("kind", list(DTYPES))
def test_cut_equals_normalize_range_of_the_sliced_or_padded_tile(kind, rng, fill, tile):
    a = _raster(kind)
    th, tw = tile
    mean, std = MEAN.to(DEV), STD.to(DEV)
    got = ops.scene_cut(torch.from_numpy(a).to(DEV), _origins(CUT_ORIGINS), tile, mean, std, *rng, fill=fill)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, 3, th, tw) and got.is_contiguous()
    pad = 16
    padded = np.pad(a, ((0, 0), (pad, pad), (pad, pad)), constant_values=fill)
    for b, (y, x) in enumerate(CUT_ORIGINS):
        cut = np.ascontiguousarray(padded[None, :, y + pad:y + pad + th, x + pad:x + pad + tw])
        want = ops.normalize_range(torch.from_numpy(cut).to(DEV), mean, std, *rng)
        assert torch.equal(got[b], want[0]), f"tile at {(y, x)} differs from normalize_range of the padded slice"
        if 0 <= y and y + th <= 37 and 0 <= x and x + tw <= 53:
            inside = np.ascontiguousarray(a[None, :, y:y + th, x:x + tw])
            assert torch.equal(got[b], ops.normalize_range(torch.from_numpy(inside).to(DEV), mean, std, *rng)[0])
    assert (0, 0) in CUT_ORIGINS and (21, 37) in CUT_ORIGINS      # the two that lie inside for the 16 x 16 tile


def test_cut_rejects_an_empty_range():
    from gdlhip import _lib
    raster = torch.from_numpy(_raster("uint8")).to(DEV)
    with pytest.raises(ValueError, match="image_max == image_min"):
        ops.scene_cut(raster, _origins(CUT_ORIGINS), (16, 16), MEAN.to(DEV), STD.to(DEV), 7, 7, 0.0, 1.0)
    out = torch.empty((4, 3, 16, 16), device=DEV)
    status = _lib.load().gdl_scene_cut(raster.data_ptr(), 0, 3, 37, 53, _origins(CUT_ORIGINS).data_ptr(), 4, 16, 16, 0, out.data_ptr(), 7, 7,
                                       0.0, 1.0, MEAN.to(DEV).data_ptr(), STD.to(DEV).data_ptr(), None)
    assert status == -1 and b"image_max == image_min (7): the range is empty" in _lib.load().gdl_last_error()


# ------------------------------------------------------------------ the blend cases
def _torch_probs(low: torch.Tensor, size) -> torch.Tensor:
    x = F.interpolate(low.permute(0, 3, 1, 2), size=tuple(size), mode="bilinear", align_corners=False)
    return x.softmax(dim=1) if x.shape[1] > 1 else x.sigmoid()


@functools.lru_cache(maxsize=None)
def _low(n: int, k: int, lo) -> torch.Tensor:
    """[n, lo, lo, k] logits of magnitude up to +-30 with the planted extremes of test_hip_inference_tail._probs_case."""
    g = torch.Generator().manual_seed(1000 * k + 10 * lo[0] + n)
    low = (torch.rand(n, lo[0], lo[1], k, generator=g) * 2 - 1) * 30
    low[0, 0, 0, :] = 30.0
    low[0, 0, 0, 0] = -30.0
    low[-1, -1, -1, :] = -30.0
    low[-1, -1, -1, -1] = 30.0
    return low


def _stitch(probs: torch.Tensor, plan: torch.Tensor, wy: torch.Tensor, wx: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """The canvas [K+1, H, W] of tiles that lie inside it, in the dtype of ``probs``: the weighted add, tile after tile."""
    K, th, tw = probs.shape[1:]
    canvas = torch.zeros(K + 1, H, W, dtype=probs.dtype)
    w2 = wy.to(probs.dtype)[:, None] * wx.to(probs.dtype)[None, :]
    for t, (y, x) in enumerate(plan.tolist()):
        assert 0 <= y <= H - th and 0 <= x <= W - tw
        canvas[:K, y:y + th, x:x + tw] += w2 * probs[t]
        canvas[K, y:y + th, x:x + tw] += w2
    return canvas


def _run_blend(route: str, low: torch.Tensor, size, plan: torch.Tensor, wy, wx, canvas: torch.Tensor, batch: int, boxed: bool = True):
    """Feeds the tiles to one of the two blend kernels in batches of ``batch``, in plan order."""
    dlow, dplan = low.to(DEV), plan.to(DEV)
    for i in range(0, plan.shape[0], batch):
        box = gscene.bounding_box(plan[i:i + batch], size) if boxed else None
        if route == "lowres":
            ops.scene_blend_lowres(dlow[i:i + batch].contiguous(), size, dplan[i:i + batch], wy, wx, canvas, box)
        else:
            ops.scene_blend(ops.upsample_probs(dlow[i:i + batch].contiguous(), size), dplan[i:i + batch], wy, wx, canvas, box)
    return canvas


# ------------------------------------------------------------------ 2. blend, anchored to the existing kernels
# 4x4 -> 16x16 an integer factor, 7x7 -> 16x16 a non-integer one; 7x7 -> 16x15: a canvas row that takes the one-pixel path
@pytest.mark.parametrize("lo,size", [((4, 4), (16, 16)), ((7, 7), (16, 16)), ((7, 7), (16, 15))], ids=["4x4-16x16", "7x7-16x16", "7x7-16x15"])
@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_one_tile_flat_window_reproduces_the_probabilities_bit_for_bit(k, lo, size):
    low = _low(1, k, lo).to(DEV)
    probs = ops.upsample_probs(low, size)
    wy, wx = gscene.window(size[0], "flat").to(DEV), gscene.window(size[1], "flat").to(DEV)
    origin = _origins([(0, 0)])
    full = ops.scene_blend(probs, origin, wy, wx, torch.zeros((k + 1, *size), device=DEV))
    assert torch.equal(full[:k], probs[0]) and torch.equal(full[k], torch.ones(size, device=DEV))
    lowres = ops.scene_blend_lowres(low, size, origin, wy, wx, torch.zeros((k + 1, *size), device=DEV))
    d = (lowres[:k] - probs[0]).abs().max().item()
    print(f"scene_blend_lowres K={k} {lo}->{size}: vs upsample_probs {d:.3e}")
    assert torch.equal(lowres[k], torch.ones(size, device=DEV))
    if size[1] % 4 == 0:
        assert torch.equal(lowres[:k], probs[0])
    else:
        # the one-pixel kernels: gdl_upsample_probs's own two kernels differ from each other in how the compiler contracts the
        # bilinear form into FMAs (measured here for K = 1: 6.0e-8, half an ulp of a probability near 1), so the one-pixel blend
        # is held to the f64 rule instead: 4 x torch's own f32 deviation, floor one ulp
        want = _torch_probs(_low(1, k, lo).double(), size)[0]
        bound, own = _bound(want, _torch_probs(_low(1, k, lo), size)[0])
        err = (lowres[:k].cpu().double() - want).abs().max().item()
        print(f"scene_blend_lowres K={k} {lo}->{size}: kernel-f64 {err:.3e}  torch f32-f64 {own:.3e}  bound {bound:.3e}")
        assert err <= bound


# ------------------------------------------------------------------ 3. blend against f64
# 37 x 53 with strides (8, 12): the one-pixel path, clamped last origins; 37 x 56 with strides (8, 10): 16-byte canvas accesses with
# tile origins that are no multiple of four
GEOMETRIES = [(37, 53, (8, 12)), (37, 56, (8, 10))]
TILE = (16, 16)


@functools.lru_cache(maxsize=None)
def _blend_case(k: int, geometry):
    H, W, stride = geometry
    plan = gscene.plan_tiles(H, W, TILE, stride)
    low = _low(plan.shape[0], k, (7, 7))
    wy, wx = gscene.window(TILE[0], "hann"), gscene.window(TILE[1], "hann")
    want = _stitch(_torch_probs(low.double(), TILE), plan, wy, wx, H, W)
    own = _stitch(_torch_probs(low, TILE), plan, wy, wx, H, W)
    return plan, low, wy, wx, want, own


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=["37x53", "37x56"])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("route", ["full", "lowres"])
def test_blend_matches_the_f64_stitch(route, k, geometry):
    H, W, _ = geometry
    plan, low, wy, wx, want, own = _blend_case(k, geometry)
    assert plan.shape[0] == 20
    got = _run_blend(route, low, TILE, plan, wy.to(DEV), wx.to(DEV), torch.zeros((k + 1, H, W), device=DEV), plan.shape[0]).cpu().double()
    for name, sl in (("probability planes", slice(0, k)), ("weight plane", slice(k, k + 1))):
        bound, own_err = _bound(want[sl], own[sl])
        err = (got[sl] - want[sl]).abs().max().item()
        print(f"scene_blend[{route}] K={k} {H}x{W} {name}: kernel-f64 {err:.3e}  torch f32-f64 {own_err:.3e}  bound {bound:.3e}  "
              f"|out| max {want[sl].abs().max().item():.3e}")
        assert err <= bound
    assert (got[k] > 0).all(), "the plan covers every pixel and the Hann window is strictly positive"


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=["37x53", "37x56"])
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("route", ["full", "lowres"])
def test_canvas_does_not_depend_on_the_batching(route, k, geometry):
    H, W, _ = geometry
    plan, low, wy, wx, _, _ = _blend_case(k, geometry)
    wy, wx = wy.to(DEV), wx.to(DEV)
    canvases = [_run_blend(route, low, TILE, plan, wy, wx, torch.zeros((k + 1, H, W), device=DEV), b) for b in (1, 3, plan.shape[0])]
    assert torch.equal(canvases[0], canvases[1]) and torch.equal(canvases[0], canvases[2])
    whole = _run_blend(route, low, TILE, plan, wy, wx, torch.zeros((k + 1, H, W), device=DEV), 3, boxed=False)
    assert torch.equal(canvases[0], whole), "the bounding box only limits the work"


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=["37x53", "37x56"])
@pytest.mark.parametrize("route", ["full", "lowres"])
def test_pixels_no_tile_of_the_batch_covers_keep_their_value(route, geometry):
    """A batch of the first and the last tile of the plan: its bounding box is the whole canvas, most of which neither covers."""
    H, W, _ = geometry
    k = 5
    plan, low, wy, wx, _, _ = _blend_case(k, geometry)
    pick = torch.tensor([0, plan.shape[0] - 1])
    sentinel = -7.5
    canvas = torch.full((k + 1, H, W), sentinel, device=DEV)
    _run_blend(route, low[pick], TILE, plan[pick], wy.to(DEV), wx.to(DEV), canvas, 2)
    covered = torch.zeros(H, W, dtype=torch.bool)
    for y, x in plan[pick].tolist():
        covered[y:y + TILE[0], x:x + TILE[1]] = True
    got = canvas.cpu()
    assert not covered[0:5, 45:50].any() and (got[:, 0:5, 45:50] == sentinel).all()
    # (a probability plane may keep the value where w * p is below half an ulp of it; the weight, at least 5.8e-6, never is)
    assert (got[:, ~covered] == sentinel).all() and (got[k, covered] != sentinel).all()


# ------------------------------------------------------------------ 5. finish
# H*W = 35: an unaligned tail, one pixel per thread; 67 x 129: several blocks; 64 x 68: four pixels per thread
FINISH_SIZES = [(5, 7), (67, 129), (64, 68)]


def _finish_canvas(k: int, H: int, W: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(100 * k + H)
    den = torch.rand(H, W, generator=g) * 3.5 + 0.5
    p = torch.rand(k, H, W, generator=g)
    canvas = torch.cat([p * den, den[None]])
    canvas[:, 2, 3] = 0.0      # a pixel no tile covered
    return canvas


@pytest.mark.parametrize("H,W", FINISH_SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("k", [3, 5, 16])
def test_finish_labels_by_arg_max(k, H, W):
    canvas = _finish_canvas(k, H, W)
    canvas[1] = canvas[0]      # the planted tie: the lower index wins
    canvas[0, 0, :] = canvas[:k, 0, :].max(0).values + 1.0      # ... also where the tied pair is the maximum
    canvas[1, 0, :] = canvas[0, 0, :]
    dev = canvas.to(DEV)
    mask, probs = ops.scene_finish(dev, return_probs=True)
    none_mask, none = ops.scene_finish(dev)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (H, W) and none is None and torch.equal(mask, none_mask)
    back = dev.cpu()
    want_mask = back[:k].argmax(0)
    assert torch.equal(mask.cpu().long(), want_mask)
    assert not (mask == 1).any() and (mask[0] == 0).all() and mask[2, 3] == 0 and (probs[:, 2, 3] == 0).all()
    want = back[:k].double() / back[k].double()
    want[:, 2, 3] = 0.0
    own = back[:k] / back[k]
    own[:, 2, 3] = 0.0
    bound, own_err = _bound(want, own)
    err = (probs.cpu().double() - want).abs().max().item()
    print(f"scene_finish K={k} {H}x{W}: kernel-f64 {err:.3e}  torch f32-f64 {own_err:.3e}  bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("H,W", FINISH_SIZES, ids=lambda v: str(v))
def test_finish_thresholds_the_one_class_quotient(H, W):
    thr = 0.5
    canvas = _finish_canvas(1, H, W)
    canvas[1, 1, 1], canvas[0, 1, 1] = 2.0, 1.0      # exactly at the threshold: not above it
    canvas[1, 1, 2], canvas[0, 1, 2] = 2.0, float(np.nextafter(np.float32(1.0), np.float32(2.0)))      # one ulp above
    dev = canvas.to(DEV)
    mask, probs = ops.scene_finish(dev, threshold=thr, return_probs=True)
    back = dev.cpu()
    want_mask = (back[0] / back[1] > thr)
    assert torch.equal(mask.cpu().bool(), want_mask) and set(mask.cpu().unique().tolist()) == {0, 1}
    assert mask[1, 1] == 0 and mask[1, 2] == 1 and mask[2, 3] == 0 and probs[0, 2, 3] == 0
    want = back[:1].double() / back[1].double()
    want[:, 2, 3] = 0.0
    own = back[:1] / back[1]
    own[:, 2, 3] = 0.0
    bound, own_err = _bound(want, own)
    err = (probs.cpu().double() - want).abs().max().item()
    print(f"scene_finish K=1 {H}x{W}: kernel-f64 {err:.3e}  torch f32-f64 {own_err:.3e}  bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------ 6. SceneInference, DOFA, end to end
@pytest.fixture(scope="module", params=[5, 1], ids=["softmax5", "sigmoid1"])
def dofa(request, golden_dir):
    """The smallest DOFA configuration of tests/test_hip_model.py (``tiny``), 3 bands, procedural weights, and a uint8 scene of
    [3, 2 img - 8, img + 5]: three tile rows (the last one clamped) by two tile columns (the second one clamped, 5 pixels on)."""
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
    g = torch.Generator().manual_seed(meta["seed"])
    scene = torch.randint(0, 256, (3, 2 * img - 8, img + 5), generator=g, dtype=torch.uint8)
    return nc, img, SegmentationScriptModel(model, **kw), model, kw, scene


def test_scene_inference_end_to_end(dofa):
    nc, img, sm, model, kw, scene = dofa
    _, H, W = scene.shape
    two, many = SceneInference(sm, tile=(img, img), overlap=0.5, batch_size=2), SceneInference(sm, tile=(img, img), overlap=0.5, batch_size=64)
    plan = gscene.plan_tiles(H, W, (img, img), two.stride)
    assert two.stride == (img // 2, img // 2) and plan.shape[0] == 6
    c2, c64 = two.canvas(scene), many.canvas(scene)
    r2 = two.predict(scene.to(DEV), return_probs=True)      # a device raster; the canvases above came from the host one
    m64, p64 = ops.scene_finish(c64, 0.5, return_probs=True)
    assert r2.mask.dtype == torch.uint8 and tuple(r2.mask.shape) == (H, W) and tuple(r2.probs.shape) == (nc, H, W)
    assert torch.equal(c2, c64) and torch.equal(r2.mask, m64) and torch.equal(r2.probs, p64)

    # the host-side stitch of script_model's probabilities of the same tiles, fed as the batches of two the first run took
    tiles = torch.stack([scene[:, y:y + img, x:x + img] for y, x in plan.tolist()])
    probs = torch.cat([sm(tiles[i:i + 2]) for i in range(0, 6, 2)]).cpu()
    wy, wx = gscene.window(img, "hann"), gscene.window(img, "hann")
    want, own = _stitch(probs.double(), plan, wy, wx, H, W), _stitch(probs, plan, wy, wx, H, W)
    got = c2.cpu().double()
    for name, sl in (("probability planes", slice(0, nc)), ("weight plane", slice(nc, nc + 1))):
        bound, own_err = _bound(want[sl], own[sl])
        err = (got[sl] - want[sl]).abs().max().item()
        print(f"SceneInference K={nc} {H}x{W} {name}: low-resolution route vs f64 stitch {err:.3e}  torch f32-f64 {own_err:.3e}  bound {bound:.3e}")
        assert err <= bound
    # the class_probs + scene_blend route is the same accumulation of the same probabilities
    full = SceneInference(sm, tile=(img, img), overlap=0.5, batch_size=2, lowres=False).canvas(scene)
    d = (full - c2).abs().max().item()
    print(f"SceneInference K={nc}: scene_blend route vs low-resolution route {d:.3e}")
    assert d <= _bound(want, own)[0]

    # a uint16 scene holding the same values is the same scene
    u16 = torch.from_numpy(scene.numpy().astype(np.uint16))
    assert torch.equal(two.canvas(u16), c2)


def test_scene_of_one_tile_with_the_flat_window_is_the_script_model(dofa):
    nc, img, sm, model, kw, scene = dofa
    raster = scene[:, :img, :img].contiguous()
    res = SceneInference(sm, tile=(img, img), window="flat").predict(raster, return_probs=True)
    want = sm(raster[None])[0]
    assert torch.equal(res.probs, want)
    want_mask = want.argmax(0) if nc > 1 else (want[0] > 0.5)
    assert torch.equal(res.mask.long(), want_mask.long())


# ------------------------------------------------------------------ 7. errors
def test_argument_errors(dofa):
    nc, img, sm, model, kw, scene = dofa
    wy, wx, origin = torch.ones(16, device=DEV), torch.ones(16, device=DEV), _origins([(0, 0)])
    low17 = torch.zeros((1, 4, 4, 17), device=DEV)
    with pytest.raises(ValueError, match="scene_blend_lowres: 1..16 classes, got 17"):
        ops.scene_blend_lowres(low17, (16, 16), origin, wy, wx, torch.zeros((18, 16, 16), device=DEV))
    from gdlhip import _lib
    status = _lib.load().gdl_scene_blend_lowres(low17.data_ptr(), 1, 4, 4, 17, 16, 16, origin.data_ptr(), wy.data_ptr(), wx.data_ptr(),
                                                torch.zeros((18, 16, 16), device=DEV).data_ptr(), 16, 16, 0, 16, 0, 16, None)
    assert status == -1 and b"gdl_scene_blend_lowres: 1..16 classes, got 17" in _lib.load().gdl_last_error()
    probs = torch.zeros((1, 5, 16, 16), device=DEV)
    with pytest.raises(ValueError, match="scene_blend: the column window wx"):
        ops.scene_blend(probs, origin, wy, torch.ones(15, device=DEV), torch.zeros((6, 16, 16), device=DEV))
    with pytest.raises(ValueError, match=r"scene_blend: canvas must be .*\[6, H, W\]"):
        ops.scene_blend(probs, origin, wy, wx, torch.zeros((5, 16, 16), device=DEV))
    with pytest.raises(ValueError, match="device tensors"):
        ops.scene_blend(probs.cpu(), origin, wy, wx, torch.zeros((6, 16, 16), device=DEV))
    with pytest.raises(ValueError, match="device tensors"):
        ops.scene_finish(torch.zeros(6, 16, 16))
    with pytest.raises(ValueError, match="device tensors"):
        ops.scene_cut(torch.zeros(3, 16, 16, dtype=torch.uint8), origin, (16, 16), MEAN.to(DEV), STD.to(DEV))
    with pytest.raises(ValueError, match="the raster has 4 channels"):
        SceneInference(sm, tile=(img, img)).predict(torch.zeros(4, img, img, dtype=torch.uint8))
