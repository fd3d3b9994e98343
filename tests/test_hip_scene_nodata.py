"""GPU tests of nodata in whole-scene inference: ``ops.scene_valid`` / ``scene_tile_valid`` / ``scene_cut_valid`` /
``scene_finish_valid`` (include/gdlhip_scene_nodata.h) and ``SceneInference(nodata=...)`` / ``predict(valid=...)``.

Every comparison is exact (``torch.equal``).  The yardsticks are torch on the host (the plane, the counts, the ``where`` that the
masked labelling adds) and the project's unmasked kernels (``scene_cut``, ``scene_cut_d4``, ``scene_finish`` and the plain
``SceneInference``), never the code under test.  Sizes as in tests/test_hip_scene.py: 37 x 53 (one pixel per thread) and 37 x 56
(four), tiles of 16 x 16 (16-byte stores) and 5 x 7 (one value per thread)."""

import functools
import json

import numpy as np
import pytest
import torch

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
H = 37
WIDTHS = [53, 56]
TILES = [(16, 16), (5, 7)]
DTYPES = {"uint8": (np.uint8, 0, 255), "uint16": (np.uint16, 0, 65535), "int16": (np.int16, -32768, 32767), "float32": (np.float32, -2000.0, 70000.0)}
MEAN = torch.tensor([0.485, 0.456, 0.406])
STD = torch.tensor([0.229, 0.224, 0.225])
NAN = float("nan")
# kind -> the nodata forms tried: one value for every band, one per band and, for f32, NaN (alone and beside numbers)
NODATA = {
    "uint8": {"one": 0, "per-band": [0, 255, 7]},
    "uint16": {"one": 0, "per-band": [0, 65535, 7]},
    "int16": {"one": -32767, "per-band": [-32767, 0, 32767]},
    "float32": {"one": -9999.0, "per-band": [-9999.0, NAN, 0.5], "nan": NAN},
}
FORMS = [(kind, form) for kind, forms in NODATA.items() for form in forms]


def _origins(pairs) -> torch.Tensor:
    return torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(DEV)


def _per_band(nodata, C: int) -> list:
    return list(nodata[:C]) if isinstance(nodata, list) else [nodata] * C


def _is_nodata(a: np.ndarray, values: list) -> torch.Tensor:
    """bool [C, H, W] on the host, the definition restated in torch: equal as floats or, for a NaN value, a NaN sample."""
    x = torch.from_numpy(a.astype(np.float32))
    return torch.stack([x[c].isnan() if v != v else x[c] == torch.tensor(v, dtype=torch.float32) for c, v in enumerate(values)])


@functools.lru_cache(maxsize=None)
def _raster(kind: str, W: int, C: int = 3) -> np.ndarray:
    """[C, 37, W] of random samples with the extreme values of the dtype."""
    npdt, lo, hi = DTYPES[kind]
    g = np.random.default_rng([29, len(kind), W, C])
    a = g.uniform(lo, hi, (C, H, W)).astype(npdt) if kind == "float32" else g.integers(lo, hi + 1, (C, H, W)).astype(npdt)
    a[:, 0, 0], a[:, 36, W - 1] = lo, hi
    return a


def _planted(kind: str, W: int, C: int, values: list) -> np.ndarray:
    """``_raster`` with nodata planted: per band in four samples of ten independently, in every band over rows 10..19 x columns
    8..29 and over the last two columns, and at (3, 5) in band 0 alone (the other bands hold something else there)."""
    a = _raster(kind, W, C).copy()
    g = np.random.default_rng([31, len(kind), W, C])
    for c, v in enumerate(values):
        hit = g.random((H, W)) < 0.4
        hit[10:20, 8:30] = True
        hit[:, W - 2:] = True
        hit[3, 5] = c == 0
        a[c][hit] = v
        if c:
            a[c, 3, 5] = 1 if v != 1 else 2
    return a


# ------------------------------------------------------------------ 1. the valid plane
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("rule", ["all", "any"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("kind,form", FORMS, ids=lambda v: str(v))
def test_valid_plane_is_the_torch_expression(kind, form, C, rule, W):
    nodata = NODATA[kind][form]
    values = _per_band(nodata, C)
    a = _planted(kind, W, C, values)
    got = ops.scene_valid(torch.from_numpy(a).to(DEV), nodata if not isinstance(nodata, list) else values, rule)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W) and got.is_contiguous()
    is_nd = _is_nodata(a, values)
    want = ~(is_nd.all(0) if rule == "all" else is_nd.any(0))
    assert torch.equal(got.cpu(), want.to(torch.uint8))
    assert not got[10:20, 8:30].any() and not got[:, W - 2:].any() and 0 < int(got.sum()) < H * W
    if C == 3:      # one band alone is nodata at (3, 5)
        assert is_nd[:, 3, 5].tolist() == [True, False, False] and int(got[3, 5]) == (1 if rule == "all" else 0)
    # the default rule is "all"
    if rule == "all":
        assert torch.equal(ops.scene_valid(torch.from_numpy(a).to(DEV), nodata if not isinstance(nodata, list) else values), got)


def test_valid_plane_of_a_view_at_an_odd_offset_takes_the_scalar_path():
    """W % 4 == 0 but a base address that is no multiple of four samples: the pointers decide, not the shape alone."""
    a = _planted("uint8", 56, 3, [0, 0, 0])
    flat = torch.zeros(a.size + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = torch.from_numpy(a).to(DEV).flatten()
    raster = flat[1:].view(3, H, 56)
    assert raster.data_ptr() % 4 == 1 and raster.is_contiguous()
    want = ~_is_nodata(a, [0, 0, 0]).all(0)
    assert torch.equal(ops.scene_valid(raster, 0).cpu(), want.to(torch.uint8))


# ------------------------------------------------------------------ 2. the counts per tile
# inside, touching the far corner, overhanging before, overhanging after, outside before, outside after, outside along one axis
COUNT_ORIGINS = [(0, 0), (21, 37), (-3, -5), (30, 45), (-20, -20), (100, 100), (5, 60), (4, 9), (17, 1)]


@functools.lru_cache(maxsize=None)
def _plane(W: int) -> torch.Tensor:
    """uint8 [37, W], half of it valid at random; rows 0..15 x columns 0..15 all valid, rows 21.. x columns 30.. all invalid."""
    g = torch.Generator().manual_seed(37 * W)
    v = (torch.rand(H, W, generator=g) < 0.5).to(torch.uint8)
    v[0:16, 0:16] = 1
    v[21:, 30:] = 0
    return v


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("tile", [*TILES, (20, 24)], ids=["16x16", "5x7", "20x24"])      # 20 x 24: more pixels than a workgroup has threads
def test_tile_counts_are_the_sums_over_the_clipped_slices(tile, W):
    th, tw = tile
    v = _plane(W)
    got = ops.scene_tile_valid(v.to(DEV), _origins(COUNT_ORIGINS), tile)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(COUNT_ORIGINS),)
    want = [int(v[max(y, 0):max(min(y + th, H), 0), max(x, 0):max(min(x + tw, W), 0)].sum()) for y, x in COUNT_ORIGINS]
    assert got.cpu().tolist() == want
    assert want[4] == 0 and want[5] == 0 and want[6] == 0      # nothing of these tiles is inside
    if tile == (16, 16):
        assert want[0] == 256 and want[1] == 0      # an all-valid tile, an all-invalid one
    # a bool plane is the same plane, and any nonzero byte counts once
    assert torch.equal(ops.scene_tile_valid(v.bool().to(DEV), _origins(COUNT_ORIGINS), tile), got)
    assert torch.equal(ops.scene_tile_valid((v * 200).to(DEV), _origins(COUNT_ORIGINS), tile), got)


def test_tile_counts_of_a_whole_plan():
    W = 56
    v = _plane(W)
    plan = gscene.plan_tiles(H, W, (16, 16), (8, 10))
    got = ops.scene_tile_valid(v.to(DEV), plan.to(DEV), (16, 16)).cpu()
    assert got.tolist() == [int(v[y:y + 16, x:x + 16].sum()) for y, x in plan.tolist()] and plan.shape[0] == 20


# ------------------------------------------------------------------ 3. the masked cut
CUT_ORIGINS = [(0, 0), (21, 37), (-3, -5), (30, 45)]      # those of tests/test_hip_scene.py
RANGES = [(0, 255, 0.0, 1.0), (-1000, 10000, -1.0, 1.0)]


def _codes(tile) -> list[int]:
    return list(range(8)) if tile[0] == tile[1] else list(range(4))


@pytest.mark.parametrize("tile", TILES, ids=["16x16", "5x7"])
@pytest.mark.parametrize("rng", RANGES, ids=lambda r: f"{r[0]}..{r[1]}")
@pytest.mark.parametrize("kind", list(DTYPES))
def test_cut_with_a_plane_of_ones_is_the_unmasked_cut(kind, rng, tile):
    raster = torch.from_numpy(_raster(kind, 53)).to(DEV)
    ones = torch.ones((H, 53), dtype=torch.uint8, device=DEV)
    mean, std, origins = MEAN.to(DEV), STD.to(DEV), _origins(CUT_ORIGINS)
    for fill in (0, 7):
        got = ops.scene_cut_valid(raster, ones, origins, None, tile, mean, std, *rng, fill=fill)
        assert got.dtype == torch.float32 and tuple(got.shape) == (4, 3, *tile) and got.is_contiguous()
        assert torch.equal(got, ops.scene_cut(raster, origins, tile, mean, std, *rng, fill=fill))
        for g in _codes(tile):
            xf = torch.full((4,), g, dtype=torch.int32, device=DEV)
            assert torch.equal(ops.scene_cut_valid(raster, ones, origins, xf, tile, mean, std, *rng, fill=fill),
                               ops.scene_cut_d4(raster, origins, xf, tile, mean, std, *rng, fill=fill)), (fill, g)
    assert torch.equal(ops.scene_cut_valid(raster, ones.bool(), origins, None, tile, mean, std, *rng), ops.scene_cut(raster, origins, tile, mean, std, *rng))


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("tile", TILES, ids=["16x16", "5x7"])
@pytest.mark.parametrize("fill", [0, 7])
@pytest.mark.parametrize("kind", list(DTYPES))
def test_cut_with_a_random_plane_is_the_cut_of_the_raster_filled_on_the_host(kind, fill, tile, W):
    a = _raster(kind, W)
    v = _plane(W)
    filled = a.copy()
    filled[:, v.numpy() == 0] = fill
    assert (filled != a).any()
    raster, want_from = torch.from_numpy(a).to(DEV), torch.from_numpy(filled).to(DEV)
    mean, std = MEAN.to(DEV), STD.to(DEV)
    rng = RANGES[1]
    codes = _codes(tile)
    # every origin without a transform, then every origin under every code: one mixed batch
    origins = _origins(CUT_ORIGINS + [o for o in CUT_ORIGINS for _ in codes])
    xforms = torch.tensor([0] * 4 + codes * 4, dtype=torch.int32, device=DEV)
    got = ops.scene_cut_valid(raster, v.to(DEV), origins, xforms, tile, mean, std, *rng, fill=fill)
    assert torch.equal(got, ops.scene_cut_d4(want_from, origins, xforms, tile, mean, std, *rng, fill=fill))
    plain = ops.scene_cut_valid(raster, v.to(DEV), origins[:4], None, tile, mean, std, *rng, fill=fill)
    assert torch.equal(plain, ops.scene_cut(want_from, origins[:4], tile, mean, std, *rng, fill=fill)) and torch.equal(plain, got[:4])
    assert not torch.equal(plain, ops.scene_cut(raster, origins[:4], tile, mean, std, *rng, fill=fill)), "the plane changes the tiles"


# ------------------------------------------------------------------ 4. the masked labelling
# H*W = 35: an unaligned tail, one pixel per thread; 67 x 129: several blocks; 64 x 68: four pixels per thread
FINISH_SIZES = [(5, 7), (67, 129), (64, 68)]


def _finish_canvas(k: int, h: int, w: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(100 * k + h)
    den = torch.rand(h, w, generator=g) * 3.5 + 0.5
    p = torch.rand(k, h, w, generator=g)
    canvas = torch.cat([p * den, den[None]])
    canvas[:, 2, 3] = 0.0      # a pixel no tile covered,
    canvas[:, 4, :] = 0.0      # a row of them,
    canvas[k, 0, 1] = 0.0      # and one whose weight alone is 0
    return canvas


@pytest.mark.parametrize("h,w", FINISH_SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("k", [1, 3, 16])
def test_finish_valid_is_finish_with_the_label_where_there_is_no_data(k, h, w):
    canvas = _finish_canvas(k, h, w).to(DEV)
    plain_mask, plain_probs = ops.scene_finish(canvas, 0.4, return_probs=True)
    covered = canvas[k] != 0
    assert not covered[4].any() and not covered[2, 3] and not covered[0, 1] and covered[1].all()
    valid = torch.rand(h, w, generator=torch.Generator().manual_seed(k + w)) < 0.6
    valid[1, 0], valid[1, 1], valid[4, 0] = True, False, True
    for plane in (None, valid.to(torch.uint8).to(DEV), valid.to(DEV), (valid.to(torch.uint8) * 255).to(DEV)):
        ok = covered if plane is None else covered & (plane != 0)
        for label in (255, 0, 9):
            mask, probs = ops.scene_finish_valid(canvas, plane, label, 0.4, return_probs=True)
            assert mask.dtype == torch.uint8 and tuple(mask.shape) == (h, w) and tuple(probs.shape) == (k, h, w)
            assert torch.equal(mask, torch.where(ok, plain_mask, torch.full_like(plain_mask, label)))
            assert torch.equal(probs, torch.where(ok, plain_probs, torch.zeros_like(plain_probs)))
            only_mask, none = ops.scene_finish_valid(canvas, plane, label, 0.4)
            assert none is None and torch.equal(only_mask, mask)
    mask = ops.scene_finish_valid(canvas, valid.to(DEV))[0]      # the default label
    assert int(mask[1, 1]) == 255 and int(mask[4, 0]) == 255 and int(mask[0, 1]) == 255 and int(mask[1, 0]) < 255


def test_argument_errors():
    raster = torch.from_numpy(_raster("uint8", 53)).to(DEV)
    mean, std, origin = MEAN.to(DEV), STD.to(DEV), _origins([(0, 0)])
    ones = torch.ones((H, 53), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match=r"scene_cut_valid: valid must be a contiguous uint8 / bool \[H, W\] = \[37, 53\]"):
        ops.scene_cut_valid(raster, ones[:, :52], origin, None, (16, 16), mean, std)
    with pytest.raises(ValueError, match="scene_cut_valid: valid must be"):
        ops.scene_cut_valid(raster, ones.float(), origin, None, (16, 16), mean, std)
    with pytest.raises(ValueError, match="device tensors"):
        ops.scene_cut_valid(raster, ones.cpu(), origin, None, (16, 16), mean, std)
    with pytest.raises(ValueError, match="scene_cut_valid: .*square tile"):
        ops.scene_cut_valid(raster, ones, origin, torch.tensor([4], dtype=torch.int32, device=DEV), (16, 12), mean, std)
    with pytest.raises(ValueError, match="scene_cut_valid: a transform code is in 0..7"):
        ops.scene_cut_valid(raster, ones, origin, torch.tensor([8], dtype=torch.int32, device=DEV), (16, 16), mean, std)
    with pytest.raises(ValueError, match="scene_cut_valid: image_max == image_min"):
        ops.scene_cut_valid(raster, ones, origin, None, (16, 16), mean, std, 7, 7)
    with pytest.raises(ValueError, match="scene_cut_valid: fill 256 is not a value"):
        ops.scene_cut_valid(raster, ones, origin, None, (16, 16), mean, std, fill=256)
    with pytest.raises(ValueError, match="scene_tile_valid: origins must be a contiguous int32"):
        ops.scene_tile_valid(ones, origin.long(), (16, 16))
    with pytest.raises(ValueError, match="scene_tile_valid: bad sizes"):
        ops.scene_tile_valid(ones, origin, (0, 16))
    canvas = torch.zeros((6, H, 53), device=DEV)
    with pytest.raises(ValueError, match="scene_finish_valid: nodata_label must be an int in 0..255, got 256"):
        ops.scene_finish_valid(canvas, ones, 256)
    with pytest.raises(ValueError, match=r"scene_finish_valid: valid must be .*\[37, 53\]"):
        ops.scene_finish_valid(canvas, ones[:36], 255)
    with pytest.raises(ValueError, match="scene_valid: .*outside 0..255"):
        ops.scene_valid(raster, -32767)
    with pytest.raises(ValueError, match="scene_valid: unknown rule"):
        ops.scene_valid(raster, 0, "most")


# ------------------------------------------------------------------ 5. SceneInference, DOFA, end to end
class _Counted:
    """Wraps ``raw_output`` of a script model: the tiles it was fed, call by call."""

    def __init__(self, sm):
        self.sm, self.inner, self.batches = sm, sm.raw_output, []

    def __enter__(self):
        def counted(tiles):
            self.batches.append(int(tiles.shape[0]))
            return self.inner(tiles)
        self.sm.raw_output = counted
        return self

    def __exit__(self, *exc):
        del self.sm.raw_output      # the instance attribute: the method is back

    @property
    def tiles(self) -> int:
        return sum(self.batches)


@pytest.fixture(scope="module", params=[5, 1], ids=["softmax5", "sigmoid1"])
def dofa(request, golden_dir):
    """The tiny DOFA recipe of tests/test_hip_scene.py and a uint8 scene [3, 3 img, 2 img] of values 1..255 with a block of zeros
    over rows 0 .. 1.5 img and columns 0 .. img: at overlap 0.5 the plan is 5 x 3 tiles, of which (0, 0) and (img / 2, 0) hold
    nothing but zeros.  With it, computed once: the plain inference (no nodata) of the scene."""
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
    sm = SegmentationScriptModel(model, **kw)
    scene = torch.randint(1, 256, (3, 3 * img, 2 * img), generator=torch.Generator().manual_seed(meta["seed"]), dtype=torch.uint8)
    scene[:, :3 * img // 2, :img] = 0
    valid = torch.ones(scene.shape[1:], dtype=torch.bool)
    valid[:3 * img // 2, :img] = False
    plain = SceneInference(sm, tile=(img, img), overlap=0.5, batch_size=64).predict(scene, return_probs=True)
    return nc, img, sm, scene, valid, plain


def _si(dofa, **kw) -> SceneInference:
    nc, img, sm, *_ = dofa
    return SceneInference(sm, tile=(img, img), overlap=0.5, **{"batch_size": 64, "fill": 0, **kw})


def _same_where_valid(res, plain, valid: torch.Tensor, label: int = 255) -> None:
    """On valid pixels the bits of ``plain``; on the others the label and probabilities 0."""
    v = valid.to(DEV)
    assert torch.equal(res.mask[v], plain.mask[v]) and torch.equal(res.probs[:, v], plain.probs[:, v])
    assert (res.mask[~v] == label).all() and not res.probs[:, ~v].any()
    assert (res.mask[v] != label).all()


def test_nodata_keeps_the_bits_of_the_valid_pixels_and_skips_the_empty_tiles(dofa):
    nc, img, sm, scene, valid, plain = dofa
    _, Hs, Ws = scene.shape
    si = _si(dofa, nodata=0)
    full = gscene.plan_tiles(Hs, Ws, (img, img), si.stride)
    assert full.shape[0] == 15
    # (b) the plan: exactly the tiles that hold nothing but nodata are dropped, the others keep their order
    kept, counts = si.tile_plan(scene)
    want_counts = [int(valid[y:y + img, x:x + img].sum()) for y, x in full.tolist()]
    assert kept.dtype == torch.int32 and counts.dtype == torch.int32 and counts.tolist() == want_counts
    empty = [o for o, n in zip(full.tolist(), want_counts) if n == 0]
    assert empty == [[0, 0], [img // 2, 0]]
    assert kept.tolist() == [o for o in full.tolist() if o not in empty] and kept.shape[0] == 13
    # (a) + (b): the model sees the kept tiles and no others
    with _Counted(sm) as seen:
        res = si.predict(scene, return_probs=True)
    assert seen.batches == [13]
    assert res.mask.dtype == torch.uint8 and tuple(res.mask.shape) == (Hs, Ws) and tuple(res.probs.shape) == (nc, Hs, Ws)
    _same_where_valid(res, plain, valid)
    # (c) the batching and the run do not matter
    with _Counted(sm) as seen:
        two = _si(dofa, nodata=0, batch_size=2).predict(scene.to(DEV), return_probs=True)
    assert seen.batches == [2] * 6 + [1]
    again = si.predict(scene, return_probs=True)
    for other in (two, again):
        assert torch.equal(other.mask, res.mask) and torch.equal(other.probs, res.probs)
    assert torch.equal(_si(dofa, nodata=0, batch_size=2).canvas(scene), si.canvas(scene))
    # (g) the same plane handed over: the same result, with and without nodata= beside it (the two are ANDed)
    for given in (valid, valid.to(torch.uint8).to(DEV)):
        for extra in ({}, {"nodata": 0}):
            explicit = _si(dofa, **extra).predict(scene, return_probs=True, valid=given)
            assert torch.equal(explicit.mask, res.mask) and torch.equal(explicit.probs, res.probs)
    k2, c2 = _si(dofa).tile_plan(scene, valid=valid)
    assert torch.equal(k2, kept) and torch.equal(c2, counts)
    # a per-band value, the "any" rule (the block is nodata in every band) and another label say the same
    other = _si(dofa, nodata=[0, 0, 0], nodata_rule="any", nodata_label=7).predict(scene, return_probs=True)
    _same_where_valid(other, plain, valid, 7)
    assert torch.equal(other.probs, res.probs)


def test_min_valid_drops_the_tiles_that_hold_too_little(dofa):
    """An island of 10 x 10 valid pixels inside the block, which tile (0, 0) alone covers: fed with ``min_valid=100``, dropped
    with 101, and then the island is valid but uncovered and takes the label."""
    nc, img, sm, scene, valid, plain = dofa
    island = valid.clone()
    island[10:20, 10:20] = True
    full = gscene.plan_tiles(scene.shape[1], scene.shape[2], (img, img), (img // 2, img // 2))
    for min_valid, tiles in ((100, 14), (101, 13)):
        si = _si(dofa, min_valid=min_valid)
        kept, counts = si.tile_plan(scene, valid=island)
        assert counts.tolist()[:4] == [100, img * img // 2, img * img, 0]
        assert kept.tolist() == [o for o, n in zip(full.tolist(), counts.tolist()) if n >= min_valid] and kept.shape[0] == tiles
        with _Counted(sm) as seen:
            res = si.predict(scene, valid=island)
        assert seen.tiles == tiles
        covered = torch.zeros_like(valid)
        for y, x in kept.tolist():
            covered[y:y + img, x:x + img] = True
        assert bool((island & ~covered).any()) == (min_valid == 101)
        assert torch.equal(res.mask.cpu() == 255, ~(island & covered))


def test_nodata_with_flips(dofa):
    """(d): the dropped tiles are dropped before the transforms multiply the rest."""
    nc, img, sm, scene, valid, plain = dofa
    plain_flips = _si(dofa, tta="flips").predict(scene, return_probs=True)
    with _Counted(sm) as seen:
        res = _si(dofa, tta="flips", nodata=0).predict(scene, return_probs=True)
    assert seen.tiles == 13 * 4
    _same_where_valid(res, plain_flips, valid)
    assert torch.equal(_si(dofa, tta="flips", nodata=0, batch_size=3).predict(scene, return_probs=True).probs, res.probs)


def test_a_scene_without_data_is_all_label_and_no_model_call(dofa):
    """(e)"""
    nc, img, sm, scene, valid, plain = dofa
    nothing = torch.zeros_like(scene)
    si = _si(dofa, nodata=0)
    kept, counts = si.tile_plan(nothing)
    assert tuple(kept.shape) == (0, 2) and counts.tolist() == [0] * 15
    with _Counted(sm) as seen:
        res = si.predict(nothing, return_probs=True)
        canvas = si.canvas(nothing)
    assert seen.batches == []
    assert (res.mask == 255).all() and not res.probs.any() and not canvas.any()
    assert tuple(res.mask.shape) == tuple(scene.shape[1:]) and tuple(res.probs.shape) == (nc, *scene.shape[1:])


def test_int16_nodata_reaches_the_model_as_fill(dofa):
    """(f): -32767 in the block, fill 0: the model sees what it sees of the raster whose block is 0."""
    nc, img, sm, scene, valid, plain = dofa
    zeroed = scene.to(torch.int16)
    marked = zeroed.clone()
    marked[:, ~valid] = -32767
    want = _si(dofa).predict(zeroed, return_probs=True)
    assert torch.equal(want.mask, plain.mask) and torch.equal(want.probs, plain.probs)      # the same values in another type
    with _Counted(sm) as seen:
        res = _si(dofa, nodata=-32767).predict(marked, return_probs=True)
    assert seen.tiles == 13
    _same_where_valid(res, want, valid)
    # without nodata= the marked raster is another scene: the huge negative samples reach the model
    assert not torch.equal(_si(dofa).predict(marked, return_probs=True).probs[:, valid.to(DEV)], want.probs[:, valid.to(DEV)])


def test_without_nodata_nothing_changes(dofa):
    """(h): no nodata and no valid plane: the canvas and the mask of the loop as it was, call for call."""
    nc, img, sm, scene, valid, plain = dofa
    _, Hs, Ws = scene.shape
    si = _si(dofa, batch_size=4)
    plan = gscene.plan_tiles(Hs, Ws, (img, img), si.stride)
    kept, counts = si.tile_plan(scene)
    assert torch.equal(kept, plan) and counts.tolist() == [img * img] * 15
    # the loop restated from the unmasked pieces
    raster, dplan = scene.to(DEV), plan.to(DEV)
    want = torch.zeros((nc + 1, Hs, Ws), device=DEV)
    for i in range(0, 15, 4):
        tiles = ops.scene_cut(raster, dplan[i:i + 4], (img, img), sm.mean, sm.std, sm.image_min, sm.image_max, sm.norm_min, sm.norm_max, 0)
        with torch.no_grad():
            si._blend(sm.raw_output(tiles), dplan[i:i + 4], want, gscene.bounding_box(plan[i:i + 4], (img, img)))
    with _Counted(sm) as seen:
        canvas = si.canvas(scene)
    assert seen.batches == [4, 4, 4, 3] and torch.equal(canvas, want)
    assert (canvas[nc] > 0).all()
    res = si.predict(scene, return_probs=True)
    mask, probs = ops.scene_finish(want, 0.5, return_probs=True)
    assert torch.equal(res.mask, mask) and torch.equal(res.probs, probs)
    assert torch.equal(res.mask, plain.mask) and torch.equal(res.probs, plain.probs)      # batches of 64 in the fixture
    # the labels of the nodata options alone switch nothing on
    idle = _si(dofa, batch_size=4, nodata_label=3, min_valid=50, nodata_rule="any").predict(scene, return_probs=True)
    assert torch.equal(idle.mask, plain.mask) and torch.equal(idle.probs, plain.probs)
