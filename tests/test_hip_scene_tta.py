"""GPU tests of test-time augmentation for whole-scene inference: ``ops.scene_cut_d4`` / ``scene_blend_d4`` /
``scene_blend_lowres_d4`` (include/gdlhip_scene_tta.h) and ``SceneInference(tta=...)``.

The transform is index arithmetic, so wherever a kernel has a counterpart without it the check is bit for bit: the cut against
``d4_apply`` of ``scene_cut``, the full-resolution blend against ``scene_blend`` of the probabilities torch permuted back, batchings
of one pair list against each other.  The low-resolution blend evaluates the probabilities itself and is held to f64 with the
rule of tests/test_hip_scene.py, restated here: the yardstick is a torch restatement in f64 on the CPU, a case's bound is 4 x the
largest deviation of the SAME restatement evaluated in f32 on the CPU from it, with a floor of one f32 ulp of the largest output
magnitude; the code under test never enters a bound, every figure is printed before it is asserted (``pytest -s``) and no pixel
is excluded.

Shapes: 16 x 16 tiles over 37 x 53 (one pixel per thread, clamped origins) and 37 x 56 (16-byte canvas accesses, origins that are
no multiple of four); 16 x 12 and 16 x 15 tiles for the codes that do not transpose; head maps of 7 x 7 and 4 x 4; K in 1, 5, 16.

Figures measured on an MI355X: in all 228 f64 comparisons of the two blends the kernel stays within 0.38 x its bound (the closest:
the low-resolution blend, K = 5, 37 x 53, code 1, 6.4e-7 against 1.7e-6); the low-resolution and the full-resolution route gave the
same canvas to the bit in all 54 cases; SceneInference with tta="d4" deviates from the f64 stitch by what torch's own f32 stitch
does (3.2e-6 .. 6.0e-6 on the probability planes, 1.6e-5 on the weight plane, sums of up to 32 pairs) against bounds of 4 x that."""

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
TILE = (16, 16)
# 37 x 53 with strides (8, 12): the one-pixel path, clamped last origins; 37 x 56 with strides (8, 10): 16-byte canvas accesses with
# tile origins that are no multiple of four (those of tests/test_hip_scene.py)
GEOMETRIES = [(37, 53, (8, 12)), (37, 56, (8, 10))]
GEO_IDS = ["37x53", "37x56"]
MIXED = "mixed"      # a different code per tile: tile t takes (3 t + 1) % 8, or % 4 for a tile that is not square


def _ulp(t: torch.Tensor) -> float:
    return float(np.spacing(np.float32(t.abs().max().item())))


def _bound(want64: torch.Tensor, own32: torch.Tensor) -> tuple[float, float]:
    """(bound, torch's own f32 deviation): 4 x own, at least one f32 ulp of the output magnitude."""
    own = (own32.double() - want64).abs().max().item()
    return max(4 * own, _ulp(want64)), own


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


def _codes(which, n: int, square: bool = True) -> torch.Tensor:
    """int32 [n] on the host: one code for every tile, or the mixed list."""
    if which == MIXED:
        return torch.tensor([(3 * t + 1) % (8 if square else 4) for t in range(n)], dtype=torch.int32)
    return torch.full((n,), int(which), dtype=torch.int32)


def _unpermute(x: torch.Tensor, codes: torch.Tensor) -> torch.Tensor:
    """Tile t of ``x`` [B, K, th, tw] taken back through the inverse of its code, by torch."""
    return torch.stack([gscene.d4_apply(x[t], gscene.d4_inverse(int(g))) for t, g in enumerate(codes.tolist())]).contiguous()


def _origins(pairs) -> torch.Tensor:
    return torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(DEV)


# ------------------------------------------------------------------ 1. cut
RANGES = {"uint8": (0, 255, 0.0, 1.0), "int16": (-1000, 10000, -1.0, 1.0)}
DTYPES = {"uint8": (np.uint8, 0, 255), "int16": (np.int16, -32768, 32767)}
MEAN = torch.tensor([0.485, 0.456, 0.406])
STD = torch.tensor([0.229, 0.224, 0.225])
CUT_ORIGINS = [(0, 0), (21, 37), (-3, -5), (30, 45)]      # inside, touching the far corner, overhanging before, overhanging after


@functools.lru_cache(maxsize=None)
def _raster(kind: str) -> torch.Tensor:
    """[3, 37, 53] on the device with the extreme values of the dtype in every channel."""
    npdt, lo, hi = DTYPES[kind]
    a = np.random.default_rng([29, len(kind)]).integers(lo, hi + 1, (3, 37, 53)).astype(npdt)
    a[:, 0, 0], a[:, 36, 52], a[:, 20, 30] = lo, hi, 0
    return torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize("g", range(8))
@pytest.mark.parametrize("kind", list(DTYPES))
def test_cut_is_the_permuted_cut(kind, g):
    raster, mean, std, origins = _raster(kind), MEAN.to(DEV), STD.to(DEV), _origins(CUT_ORIGINS)
    # 16 x 16: 16-byte stores; 16 x 12: the same, not square; 16 x 15: one value per thread
    for tile in [(16, 16)] + ([] if g & 4 else [(16, 12), (16, 15)]):
        plain = ops.scene_cut(raster, origins, tile, mean, std, *RANGES[kind], fill=7)
        got = ops.scene_cut_d4(raster, origins, _codes(g, 4).to(DEV), tile, mean, std, *RANGES[kind], fill=7)
        assert got.dtype == torch.float32 and tuple(got.shape) == (4, 3, *tile) and got.is_contiguous()
        assert torch.equal(got, gscene.d4_apply(plain, g)), f"code {g}, tile {tile}"
        if g:
            assert not torch.equal(got, plain)


@pytest.mark.parametrize("kind", list(DTYPES))
def test_cut_of_a_mixed_batch_equals_the_tiles_cut_one_by_one(kind):
    raster, mean, std = _raster(kind), MEAN.to(DEV), STD.to(DEV)
    origins, codes = _origins(CUT_ORIGINS * 2), torch.arange(8, dtype=torch.int32)
    got = ops.scene_cut_d4(raster, origins, codes.to(DEV), TILE, mean, std, *RANGES[kind], fill=7)
    plain = ops.scene_cut(raster, origins, TILE, mean, std, *RANGES[kind], fill=7)
    for b, g in enumerate(codes.tolist()):
        one = ops.scene_cut_d4(raster, origins[b:b + 1], codes[b:b + 1].to(DEV), TILE, mean, std, *RANGES[kind], fill=7)
        assert torch.equal(got[b], one[0]) and torch.equal(got[b], gscene.d4_apply(plain[b], g)), f"tile {b}, code {g}"


# ------------------------------------------------------------------ the blend cases
def _torch_probs(low: torch.Tensor, size) -> torch.Tensor:
    x = F.interpolate(low.permute(0, 3, 1, 2), size=tuple(size), mode="bilinear", align_corners=False)
    return x.softmax(dim=1) if x.shape[1] > 1 else x.sigmoid()


@functools.lru_cache(maxsize=None)
def _low(n: int, k: int, lo) -> torch.Tensor:
    """[n, lo, lo, k] logits of magnitude up to +-30 with planted extremes in the first and the last tile."""
    g = torch.Generator().manual_seed(2000 * k + 10 * lo[0] + n)
    low = (torch.rand(n, lo[0], lo[1], k, generator=g) * 2 - 1) * 30
    low[0, 0, 0, :] = 30.0
    low[0, 0, 0, 0] = -30.0
    low[-1, -1, -1, :] = -30.0
    low[-1, -1, -1, -1] = 30.0
    return low


@functools.lru_cache(maxsize=None)
def _case(k: int, geometry, which, lo=(7, 7), tile=TILE):
    """One pair list and its yardsticks, computed once: the plan, the codes, the maps of the TRANSFORMED tiles, the windows and
    the f64 / f32 stitches of torch's probabilities taken back through the inverse transforms."""
    H, W, stride = geometry
    plan = gscene.plan_tiles(H, W, tile, stride)
    codes = _codes(which, plan.shape[0], tile[0] == tile[1])
    low = _low(plan.shape[0], k, lo)
    wy, wx = gscene.window(tile[0], "hann"), gscene.window(tile[1], "hann")
    want = _stitch(_unpermute(_torch_probs(low.double(), tile), codes), plan, wy, wx, H, W)
    own = _stitch(_unpermute(_torch_probs(low, tile), codes), plan, wy, wx, H, W)
    return plan, codes, low, wy, wx, want, own


def _run(route: str, low: torch.Tensor, size, plan: torch.Tensor, codes: torch.Tensor, wy, wx, canvas: torch.Tensor, batch: int,
         boxed: bool = True) -> torch.Tensor:
    """Feeds the pairs to one of the two D4 blend kernels in batches of ``batch``, in list order."""
    dlow, dplan, dcodes = low.to(DEV), plan.to(DEV), codes.to(DEV)
    for i in range(0, plan.shape[0], batch):
        box = gscene.bounding_box(plan[i:i + batch], size) if boxed else None
        part = dlow[i:i + batch].contiguous()
        if route == "lowres":
            ops.scene_blend_lowres_d4(part, size, dplan[i:i + batch], dcodes[i:i + batch], wy, wx, canvas, box)
        else:
            ops.scene_blend_d4(ops.upsample_probs(part, size), dplan[i:i + batch], dcodes[i:i + batch], wy, wx, canvas, box)
    return canvas


# ------------------------------------------------------------------ 2. full-resolution blend, exact
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GEO_IDS)
@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("which", [*range(8), MIXED], ids=str)
def test_full_resolution_blend_is_scene_blend_of_the_unpermuted_probabilities(which, k, geometry):
    H, W, stride = geometry
    for tile in [TILE] + ([(16, 12), (16, 15)] if which == MIXED or not which & 4 else []):
        plan = gscene.plan_tiles(H, W, tile, stride)
        n = plan.shape[0]
        codes = _codes(which, n, tile[0] == tile[1])
        probs = torch.rand(n, k, *tile, generator=torch.Generator().manual_seed(31 * k + n))      # the transformed frame
        wy, wx = gscene.window(tile[0], "hann").to(DEV), gscene.window(tile[1], "hann").to(DEV)
        dplan, box = plan.to(DEV), gscene.bounding_box(plan, tile)
        got = ops.scene_blend_d4(probs.to(DEV), dplan, codes.to(DEV), wy, wx, torch.zeros((k + 1, H, W), device=DEV), box)
        want = ops.scene_blend(_unpermute(probs, codes).to(DEV), dplan, wy, wx, torch.zeros((k + 1, H, W), device=DEV), box)
        assert torch.equal(got, want), f"codes {which}, tile {tile}"
        assert (got[k] > 0).all(), "the plan covers every pixel and the Hann window is strictly positive"
        if which == 0:
            same = ops.scene_blend(probs.to(DEV), dplan, wy, wx, torch.zeros((k + 1, H, W), device=DEV), box)
            assert torch.equal(got, same), "all-zero codes are scene_blend"
        else:
            plain = ops.scene_blend(probs.to(DEV), dplan, wy, wx, torch.zeros((k + 1, H, W), device=DEV), box)
            assert not torch.equal(got[:k], plain[:k]) and torch.equal(got[k], plain[k]), "the weights do not move with the tile"


# ------------------------------------------------------------------ 3. low-resolution blend against f64
def _check_against_f64(label: str, got: torch.Tensor, want: torch.Tensor, own: torch.Tensor, k: int) -> None:
    for name, sl in (("probability planes", slice(0, k)), ("weight plane", slice(k, k + 1))):
        bound, own_err = _bound(want[sl], own[sl])
        err = (got[sl] - want[sl]).abs().max().item()
        print(f"{label} {name}: kernel-f64 {err:.3e}  torch f32-f64 {own_err:.3e}  bound {bound:.3e}  |out| max {want[sl].abs().max().item():.3e}")
        assert err <= bound


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GEO_IDS)
@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("which", [*range(8), MIXED], ids=str)
def test_low_resolution_blend_matches_the_f64_stitch(which, k, geometry):
    H, W, _ = geometry
    plan, codes, low, wy, wx, want, own = _case(k, geometry, which)
    assert plan.shape[0] == 20
    zeros = lambda: torch.zeros((k + 1, H, W), device=DEV)      # noqa: E731
    got = _run("lowres", low, TILE, plan, codes, wy.to(DEV), wx.to(DEV), zeros(), plan.shape[0])
    full = _run("full", low, TILE, plan, codes, wy.to(DEV), wx.to(DEV), zeros(), plan.shape[0])
    print(f"scene_blend_lowres_d4 K={k} {H}x{W} codes {which}: vs upsample_probs + scene_blend_d4 {(got - full).abs().max().item():.3e}")
    _check_against_f64(f"scene_blend_lowres_d4 K={k} {H}x{W} codes {which}", got.cpu().double(), want, own, k)
    _check_against_f64(f"scene_blend_d4 K={k} {H}x{W} codes {which}", full.cpu().double(), want, own, k)
    assert (got[k] > 0).all()


# 4 x 4 -> 16 x 16: an integer factor; 7 x 7 -> 16 x 12 and 16 x 15: tiles that are not square (flips only), the second on the
# one-pixel path whatever the canvas
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GEO_IDS)
@pytest.mark.parametrize("lo,tile", [((4, 4), (16, 16)), ((7, 7), (16, 12)), ((7, 7), (16, 15))], ids=["4x4-16x16", "7x7-16x12", "7x7-16x15"])
def test_low_resolution_blend_of_other_maps_and_tiles(lo, tile, geometry):
    H, W, _ = geometry
    k = 5
    plan, codes, low, wy, wx, want, own = _case(k, geometry, MIXED, lo, tile)
    assert set(codes.tolist()) == (set(range(8)) if tile[0] == tile[1] else set(range(4)))
    got = _run("lowres", low, tile, plan, codes, wy.to(DEV), wx.to(DEV), torch.zeros((k + 1, H, W), device=DEV), plan.shape[0])
    _check_against_f64(f"scene_blend_lowres_d4 K={k} {H}x{W} {lo}->{tile}", got.cpu().double(), want, own, k)


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GEO_IDS)
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("route", ["full", "lowres"])
def test_canvas_does_not_depend_on_the_batching(route, k, geometry):
    H, W, _ = geometry
    base, _, _, wy, wx, _, _ = _case(k, geometry, MIXED)
    plan, codes = gscene.plan_tta(base[:6], (0, 6, 3, 5))      # 24 pairs: four transforms of each of six tiles
    low = _low(plan.shape[0], k, (7, 7))
    wy, wx = wy.to(DEV), wx.to(DEV)
    zeros = lambda: torch.zeros((k + 1, H, W), device=DEV)      # noqa: E731
    canvases = [_run(route, low, TILE, plan, codes, wy, wx, zeros(), b) for b in (1, 3, plan.shape[0])]
    assert torch.equal(canvases[0], canvases[1]) and torch.equal(canvases[0], canvases[2])
    whole = _run(route, low, TILE, plan, codes, wy, wx, zeros(), 3, boxed=False)
    assert torch.equal(canvases[0], whole), "the bounding box only limits the work"
    assert (canvases[0][k] > 0).any() and (canvases[0][k] == 0).any()      # six tiles do not cover the canvas


# ------------------------------------------------------------------ 5. uncovered pixels
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GEO_IDS)
@pytest.mark.parametrize("route", ["full", "lowres"])
def test_pixels_no_pair_of_the_batch_covers_keep_their_value(route, geometry):
    """A batch of the first and the last pair of the list: its bounding box is the whole canvas, most of which neither covers."""
    H, W, _ = geometry
    k = 5
    plan, codes, low, wy, wx, _, _ = _case(k, geometry, MIXED)
    pick = torch.tensor([0, plan.shape[0] - 1])
    assert codes[pick].tolist() == [1, 2]
    sentinel = -7.5
    canvas = torch.full((k + 1, H, W), sentinel, device=DEV)
    _run(route, low[pick], TILE, plan[pick], codes[pick], wy.to(DEV), wx.to(DEV), canvas, 2)
    covered = torch.zeros(H, W, dtype=torch.bool)
    for y, x in plan[pick].tolist():
        covered[y:y + TILE[0], x:x + TILE[1]] = True
    got = canvas.cpu()
    assert not covered[0:5, 45:50].any() and (got[:, 0:5, 45:50] == sentinel).all()
    # (a probability plane may keep the value where w * p is below half an ulp of it; the weight, at least 5.8e-6, never is)
    assert (got[:, ~covered] == sentinel).all() and (got[k, covered] != sentinel).all()


# ------------------------------------------------------------------ 6. SceneInference, DOFA, end to end
@pytest.fixture(scope="module", params=[5, 1], ids=["softmax5", "sigmoid1"])
def dofa(request, golden_dir):
    """The tiny DOFA recipe of tests/test_hip_scene.py: 3 bands, procedural weights, and a uint8 scene of [3, 2 img - 8, img + 5]:
    three tile rows (the last one clamped) by two tile columns (the second one clamped, 5 pixels on).  With it, computed once, the
    canvases without augmentation on both routes and the f64 / f32 host stitches of the script model's probabilities."""
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
    scene = torch.randint(0, 256, (3, 2 * img - 8, img + 5), generator=torch.Generator().manual_seed(meta["seed"]), dtype=torch.uint8)
    sm = SegmentationScriptModel(model, **kw)
    _, H, W = scene.shape
    plan = gscene.plan_tiles(H, W, (img, img), (img // 2, img // 2))
    assert plan.shape[0] == 6
    tiles = torch.stack([scene[:, y:y + img, x:x + img] for y, x in plan.tolist()])
    probs = torch.cat([sm(tiles[i:i + 3]) for i in range(0, 6, 3)]).cpu()
    wy = wx = gscene.window(img, "hann")
    plain = (_stitch(probs.double(), plan, wy, wx, H, W), _stitch(probs, plan, wy, wx, H, W))
    return nc, img, sm, scene, plan, tiles, plain


def _si(dofa, **kw) -> SceneInference:
    nc, img, sm, *_ = dofa
    return SceneInference(sm, tile=(img, img), overlap=0.5, **{"batch_size": 3, **kw})


def test_scene_inference_with_the_identity_alone_is_scene_inference(dofa):
    nc, img, sm, scene, plan, tiles, (want, own) = dofa
    assert _si(dofa, tta=(0,)).tta == (0,) and _si(dofa).tta is None and _si(dofa, tta="none").tta == (0,)
    full_none, full_id = _si(dofa, lowres=False).canvas(scene), _si(dofa, lowres=False, tta=(0,)).canvas(scene)
    assert torch.equal(full_none, full_id), "scene_cut_d4 + scene_blend_d4 with code 0 are scene_cut + scene_blend, bit for bit"
    low_none, low_id = _si(dofa).canvas(scene), _si(dofa, tta=(0,)).canvas(scene)
    d = (low_none - low_id).abs().max().item()
    bound = _bound(want, own)[0]
    print(f"SceneInference K={nc}: tta=(0,) vs tta=None on the low-resolution route {d:.3e}  bound {bound:.3e}")
    assert d <= bound
    _check_against_f64(f"SceneInference K={nc} tta=(0,)", low_id.cpu().double(), want, own, nc)


def test_scene_inference_d4_end_to_end(dofa):
    nc, img, sm, scene, plan, tiles, (want0, own0) = dofa
    _, H, W = scene.shape
    three, many = _si(dofa, tta="d4"), _si(dofa, tta="d4", batch_size=64)
    assert three.tta == gscene.D4
    c3, c64 = three.canvas(scene), many.canvas(scene)
    assert torch.equal(c3, c64)
    res = three.predict(scene.to(DEV), return_probs=True)
    assert res.mask.dtype == torch.uint8 and tuple(res.mask.shape) == (H, W) and tuple(res.probs.shape) == (nc, H, W)
    m64, p64 = ops.scene_finish(c64, 0.5, return_probs=True)
    assert torch.equal(res.mask, m64) and torch.equal(res.probs, p64)

    # the host stitch: the script model on the torch-permuted tile of every pair, in the batches of three the first run took, its
    # probabilities taken back by torch
    origins, codes = gscene.plan_tta(plan, gscene.D4)
    assert origins.shape[0] == 48
    fed = torch.stack([gscene.d4_apply(tiles[t // 8], int(g)) for t, g in enumerate(codes.tolist())]).contiguous()
    probs = _unpermute(torch.cat([sm(fed[i:i + 3]) for i in range(0, 48, 3)]).cpu(), codes)
    wy = wx = gscene.window(img, "hann")
    want, own = _stitch(probs.double(), origins, wy, wx, H, W), _stitch(probs, origins, wy, wx, H, W)
    _check_against_f64(f"SceneInference K={nc} {H}x{W} tta=d4, low-resolution route", c3.cpu().double(), want, own, nc)

    # eight transforms of a tile weigh eight times the tile
    wbound = _bound(want[nc:], own[nc:])[0]
    derr = (c3[nc].cpu().double() - 8 * want0[nc]).abs().max().item()
    print(f"SceneInference K={nc} tta=d4: weights plane vs 8 x the plain one {derr:.3e}  bound {wbound:.3e}")
    assert derr <= wbound
    assert (8 * _si(dofa).canvas(scene)[nc].cpu().double() - c3[nc].cpu().double()).abs().max().item() <= wbound

    # the class_probs + scene_blend_d4 route is the same accumulation of the same probabilities
    full = _si(dofa, tta="d4", lowres=False).canvas(scene)
    d = (full - c3).abs().max().item()
    bound = _bound(want, own)[0]
    print(f"SceneInference K={nc} tta=d4: scene_blend_d4 route vs low-resolution route {d:.3e}  bound {bound:.3e}")
    assert d <= bound
    _check_against_f64(f"SceneInference K={nc} {H}x{W} tta=d4, full-resolution route", full.cpu().double(), want, own, nc)


# ------------------------------------------------------------------ 7. errors
def test_argument_errors(dofa):
    nc, img, sm, scene, *_ = dofa
    raster, mean, std = _raster("uint8"), MEAN.to(DEV), STD.to(DEV)
    wy, wx12, origin = torch.ones(16, device=DEV), torch.ones(12, device=DEV), _origins([(0, 0)])
    code = lambda g: torch.tensor([g], dtype=torch.int32, device=DEV)      # noqa: E731
    probs12, canvas12 = torch.zeros((1, 5, 16, 12), device=DEV), torch.zeros((6, 16, 12), device=DEV)
    # a code that transposes, a tile that is not square: refused on the host, nothing is launched and nothing is written
    for g in (4, 5, 6, 7):
        with pytest.raises(ValueError, match="scene_cut_d4: .*square tile"):
            ops.scene_cut_d4(raster, origin, code(g), (16, 12), mean, std)
        with pytest.raises(ValueError, match="scene_blend_d4: .*square tile"):
            ops.scene_blend_d4(probs12 + 1, origin, code(g), wy, wx12, canvas12)
        with pytest.raises(ValueError, match="scene_blend_lowres_d4: .*square tile"):
            ops.scene_blend_lowres_d4(torch.zeros((1, 4, 4, 5), device=DEV), (16, 12), origin, code(g), wy, wx12, canvas12)
    assert not canvas12.any()
    for bad in (8, -1):
        with pytest.raises(ValueError, match="scene_cut_d4: a transform code is in 0..7"):
            ops.scene_cut_d4(raster, origin, code(bad), (16, 16), mean, std)
    ops.scene_cut_d4(raster, origin, code(3), (16, 12), mean, std)      # a flip of a tile that is not square is fine
    # xforms of the wrong length, of the wrong dtype, on the host
    with pytest.raises(ValueError, match="scene_cut_d4: 2 transform codes for 1 tiles"):
        ops.scene_cut_d4(raster, origin, torch.zeros(2, dtype=torch.int32, device=DEV), (16, 16), mean, std)
    with pytest.raises(ValueError, match="scene_blend_d4: xforms must be a contiguous int32"):
        ops.scene_blend_d4(probs12, origin, torch.zeros(1, dtype=torch.int64, device=DEV), wy, wx12, canvas12)
    with pytest.raises(ValueError, match="scene_blend_lowres_d4: xforms must be a contiguous int32"):
        ops.scene_blend_lowres_d4(torch.zeros((1, 4, 4, 5), device=DEV), (16, 12), origin, torch.zeros((1, 1), dtype=torch.int32, device=DEV),
                                  wy, wx12, canvas12)
    for call in (lambda x: ops.scene_cut_d4(raster, origin, x, (16, 16), mean, std),
                 lambda x: ops.scene_blend_d4(probs12, origin, x, wy, wx12, canvas12),
                 lambda x: ops.scene_blend_lowres_d4(torch.zeros((1, 4, 4, 5), device=DEV), (16, 12), origin, x, wy, wx12, canvas12)):
        with pytest.raises(ValueError, match="device tensors"):
            call(torch.zeros(1, dtype=torch.int32))
    # the checks of the counterparts
    low17 = torch.zeros((1, 4, 4, 17), device=DEV)
    with pytest.raises(ValueError, match="scene_blend_lowres_d4: 1..16 classes, got 17"):
        ops.scene_blend_lowres_d4(low17, (16, 16), origin, code(0), wy, wy, torch.zeros((18, 16, 16), device=DEV))
    from gdlhip import _lib
    status = _lib.load().gdl_scene_blend_lowres_d4(low17.data_ptr(), 1, 4, 4, 17, 16, 16, origin.data_ptr(), code(0).data_ptr(), wy.data_ptr(),
                                                   wy.data_ptr(), torch.zeros((18, 16, 16), device=DEV).data_ptr(), 16, 16, 0, 16, 0, 16, None)
    assert status == -1 and b"gdl_scene_blend_lowres_d4: 1..16 classes, got 17" in _lib.load().gdl_last_error()
    with pytest.raises(ValueError, match="scene_blend_d4: the column window wx"):
        ops.scene_blend_d4(probs12, origin, code(0), wy, wy, canvas12)
    with pytest.raises(ValueError, match=r"scene_blend_d4: canvas must be .*\[6, H, W\]"):
        ops.scene_blend_d4(probs12, origin, code(0), wy, wx12, torch.zeros((5, 16, 12), device=DEV))
    with pytest.raises(ValueError, match="image_max == image_min"):
        ops.scene_cut_d4(raster, origin, code(0), (16, 16), mean, std, 7, 7, 0.0, 1.0)
    # SceneInference
    with pytest.raises(ValueError, match="unknown tta 'd8'"):
        SceneInference(sm, tile=(img, img), tta="d8")
    with pytest.raises(ValueError, match="square tile"):
        SceneInference(sm, tile=(img, img - 4), tta="d4")
    with pytest.raises(ValueError, match="repeated"):
        SceneInference(sm, tile=(img, img), tta=(0, 1, 1))
