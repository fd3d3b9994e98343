"""GPU tests of the per-region attributes of whole-scene inference: ``ops.scene_regions`` (include/gdlhip_scene_regions.h),
``SceneInference.predict_features`` and ``gdlhip.scene.polygons(..., regions=)``.

Every comparison is exact.  The yardstick is the numpy restatement of tests/_regions_oracle.py (which
tests/test_scene_regions_host.py holds against scipy and against results written out by hand) on the labels of
tests/_sieve_oracle.py, computed once per mask and shared.  The oracle's probabilities are those ``ops.scene_finish`` writes
for the same canvas, so the oracle is held to the kernel's own quotient and to nothing else.  Shapes as in
tests/test_hip_scene_sieve.py: the kernel's tile is 64 x 64, so 197 x 131 and 131 x 197 cross tile edges both ways with
remainders, 37 x 53 lies inside one tile, and 1 x W, H x 1 and 1 x 1 are the degenerate rasters.

The masks are the patterns taken modulo 5, so that a canvas of five classes has a plane for every value (and one of a single
class has none for the values 2, 3, 4); ``test_values_without_a_plane`` takes the two patterns with larger values as they are.

What the named patterns reach at 197 x 131 (``test_the_named_cases_reach_what_they_are_for``), against the table of
GDL_SCENE_REGIONS_TABLE = 1024 labels a workgroup keeps in LDS:
  * constant: one region in all 12 tiles, every workgroup adds to the same nine words;
  * checkerboard, connectivity 4: 4096 labels in a full tile, so three runs in four take the fallback;
  * spiral: the arm is one region with pixels in every tile;
  * random-5: 2467 .. 2526 labels in a full tile under connectivity 4 (1499 .. 1545 under 8) -- thousands, not the hundreds one
    might guess, because a component of five random classes has fewer than two pixels on average: there the table fills up and
    the table and the fallback work side by side in one workgroup.  Its tiles on the right and lower rim hold 128 .. 204
    labels: hundreds, the table in use and nowhere near full;
  * percolation, connectivity 4: 552 .. 576 labels in every full tile, the table in use and never full, which is the case
    random-5 was meant to be."""

import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
import _regions_oracle as rg  # noqa: E402
import _sieve_oracle as so  # noqa: E402
import oracle  # noqa: E402
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402
from gdlhip import scene as gscene  # noqa: E402
from geo_deep_learning.models.encoders.dofa_v2 import DOFAv2  # noqa: E402
from geo_deep_learning.models.segmentation.dofa import DOFASegmentationModel  # noqa: E402
from geo_deep_learning.tools.scene_inference import SceneFeatures, SceneInference  # noqa: E402
from geo_deep_learning.tools.script_model import SegmentationScriptModel  # noqa: E402
from oracle import procedural_state_dict, synthetic_batch  # noqa: E402
from oracle.model import RGB_MEAN, RGB_STD  # noqa: E402

DEV = "cuda"
TILE = _lib.SCENE_REGIONS_TILE
TABLE = _lib.SCENE_REGIONS_TABLE
SHAPES = [(197, 131), (131, 197), (37, 53), (1, 200), (200, 1), (1, 1)]
PATTERNS = so.patterns(TILE)
CONNECTIVITY = [4, 8]
shape_ids = [f"{h}x{w}" for h, w in SHAPES]


@functools.lru_cache(maxsize=None)
def _mask(name: str, H: int, W: int, modulo: int | None = 5) -> np.ndarray:
    m = PATTERNS[name][0](H, W)
    m = m if modulo is None else (m % modulo).astype(np.uint8)
    m.setflags(write=False)
    return m


def _ignores(name: str, modulo: int | None = 5):
    ign = PATTERNS[name][1]
    return (None, ign if modulo is None else ign % modulo)


@functools.lru_cache(maxsize=None)
def _labels(name: str, H: int, W: int, connectivity: int, ignore, modulo: int | None = 5):
    """The oracle's (labels, sizes) of a mask, computed once."""
    labels, sizes = so.components(_mask(name, H, W, modulo), connectivity, -1 if ignore is None else ignore)
    labels.setflags(write=False)
    sizes.setflags(write=False)
    return labels, sizes


@functools.lru_cache(maxsize=None)
def _canvas(H: int, W: int, K: int):
    """(canvas f32 [K + 1, H, W] on the device, the probabilities ``scene_finish`` gives for it and its weight plane on the host):
    random positive planes, a block of weight 0, every 17th pixel with all planes equal to the weight (p = 1) and every 19th
    with all planes 0."""
    g = np.random.default_rng([23, H, W, K])
    planes = g.uniform(0.05, 1.0, (K, H, W)).astype(np.float32)
    weight = g.uniform(0.5, 3.0, (H, W)).astype(np.float32)
    weight[H // 3:H // 3 + 5, W // 4:W // 4 + 9] = 0
    flat = np.arange(H * W).reshape(H, W)
    planes = np.where(flat % 17 == 3, weight, planes)
    planes = np.where(flat % 19 == 5, np.float32(0), planes).astype(np.float32)
    canvas = torch.from_numpy(np.concatenate([planes, weight[None]])).to(DEV)
    probs = ops.scene_finish(canvas, return_probs=True)[1].cpu().numpy()
    probs.setflags(write=False)
    weight.setflags(write=False)
    return canvas, probs, weight


def _host(regions: ops.SceneRegions) -> rg.Regions:
    return rg.Regions(*(None if f is None else f.cpu().numpy() for f in regions))


def _check_form(regions: ops.SceneRegions, conf: bool) -> int:
    N = int(regions.label.numel())
    dtypes = dict(label=torch.int32, value=torch.uint8, pixels=torch.int32, bbox=torch.int32, sum_xy=torch.int64, conf_sum=torch.int64,
                  conf_min=torch.int32)
    shapes = dict(bbox=(N, 4), sum_xy=(N, 2))
    for name, t in zip(regions._fields, regions):
        if name.startswith("conf") and not conf:
            assert t is None
            continue
        assert t.dtype == dtypes[name] and tuple(t.shape) == shapes.get(name, (N,)) and t.is_contiguous() and t.is_cuda, name
    return N


def _same(a: ops.SceneRegions, b: ops.SceneRegions) -> bool:
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. ops.scene_regions against the oracle
@pytest.mark.parametrize("H,W", SHAPES, ids=shape_ids)
@pytest.mark.parametrize("name", list(PATTERNS))
def test_regions_are_the_oracles(name, H, W):
    host = _mask(name, H, W)
    mask = torch.from_numpy(host.copy()).to(DEV)
    for connectivity in CONNECTIVITY:
        for ignore in _ignores(name):
            want_labels, want_sizes = _labels(name, H, W, connectivity, ignore)
            labels, sizes = ops.scene_components(mask, connectivity, ignore)
            for K in (5, 1, None):
                where = (name, H, W, connectivity, ignore, K)
                canvas, probs, weight = _canvas(H, W, K) if K else (None, None, None)
                kept = None if canvas is None else canvas.clone()
                got = ops.scene_regions(mask, connectivity, ignore, canvas=canvas)
                N = _check_form(got, K is not None)
                want = rg.regions(host, want_labels, probs, weight)
                assert rg.same(_host(got), want), where
                assert N == int((want_sizes > 0).sum()), where
                if N:      # the pixel counts are the sizes of the components
                    assert torch.equal(got.pixels, sizes[got.label.long()]), where
                    assert int(got.pixels.sum()) == int((want_labels >= 0).sum()), where
                assert _same(ops.scene_regions(mask, connectivity, ignore, canvas=canvas), got), where      # the same bits again
                assert _same(ops.scene_regions(mask, connectivity, ignore, canvas=canvas, labels=labels), got), where
                assert canvas is None or torch.equal(canvas, kept), where
            assert np.array_equal(labels.cpu().numpy(), want_labels), "the caller's labels are not modified"
    assert np.array_equal(mask.cpu().numpy(), host), "the mask is not modified"


SCAN_TILE = _lib.SCENE_REGIONS_SCAN_TILE


@pytest.mark.parametrize("H,W,blocks", [(23, 89, "T - 1"), (32, 64, "T"), (3, 683, "T + 1"), (17, 241, "2 T + 1")])
def test_the_scan_of_the_roots_at_its_block_boundaries(H, W, blocks):
    """gdl_scene_regions_count scans H * W root flags in blocks of SCAN_TILE: a last block that is full but for one entry, exactly
    full, of one entry, and a third block of one entry.  random-5 has a root in most positions, the last pixels included, so a
    rank that is off by one block sum moves ``label`` and ``pixels``."""
    assert H * W == {"T - 1": SCAN_TILE - 1, "T": SCAN_TILE, "T + 1": SCAN_TILE + 1, "2 T + 1": 2 * SCAN_TILE + 1}[blocks]
    host = _mask("random-5", H, W)
    want = rg.regions(host, _labels("random-5", H, W, 4, None)[0])
    assert len(want.label) > H * W // 4 and want.label[-1] >= H * W - W, "roots up to the last row"
    got = _host(ops.scene_regions(torch.from_numpy(host.copy()).to(DEV)))
    assert np.array_equal(got.label, want.label) and np.array_equal(got.pixels, want.pixels) and rg.same(got, want)


@pytest.mark.parametrize("name", ["constant", "ignore-cross"])
def test_values_without_a_plane(name):
    """The patterns as they are: 7 everywhere, and a cross of 255 -- values a canvas of five classes (or of one) has no plane for."""
    H, W = 131, 197
    host = _mask(name, H, W, None)
    assert host.max() >= 5
    mask = torch.from_numpy(host.copy()).to(DEV)
    for ignore in _ignores(name, None):
        want_labels = _labels(name, H, W, 4, ignore, None)[0]
        for K in (5, 1):
            canvas, probs, weight = _canvas(H, W, K)
            got = _host(ops.scene_regions(mask, 4, ignore, canvas=canvas))
            assert rg.same(got, rg.regions(host, want_labels, probs, weight)), (name, ignore, K)
            beyond = got.value >= (5 if K == 5 else 2)
            assert ignore is not None or beyond.any()
            assert (got.conf_sum[beyond] == 0).all() and (got.conf_min[beyond] == 0).all()


@pytest.mark.parametrize("name,mask,kw,probs,weight,want", rg.HAND_CASES, ids=[c[0] for c in rg.HAND_CASES])
def test_regions_on_the_hand_drawn_cases(name, mask, kw, probs, weight, want):
    """``probs`` of a hand case are multiples of 1 / 4 and its weights 0 or 1, so probs * weight is a canvas whose quotient gives
    them back exactly."""
    canvas = None if probs is None else torch.from_numpy(np.concatenate([probs * weight, weight[None]]).astype(np.float32)).to(DEV)
    got = ops.scene_regions(torch.from_numpy(mask.copy()).to(DEV), kw.get("connectivity", 4), kw.get("ignore_label"), canvas=canvas)
    assert rg.same(_host(got), want), f"\n{_host(got)}"


def test_the_named_cases_reach_what_they_are_for():
    H, W = SHAPES[0]
    tiles = -(-H // TILE) * -(-W // TILE)
    full = [t for t in range(tiles) if (t // -(-W // TILE) + 1) * TILE <= H and (t % -(-W // TILE) + 1) * TILE <= W]
    assert tiles == 12 and len(full) == 6 and TABLE < TILE * TILE
    counts = lambda name, c: rg.tile_label_counts(_labels(name, H, W, c, None)[0], TILE)      # noqa: E731

    # the constant mask with p = 1 everywhere: one region spanning every tile, and no update is lost under contention
    const = torch.from_numpy(_mask("constant", H, W).copy()).to(DEV)
    weight = torch.rand((1, H, W), device=DEV) + 0.5
    assert int(const[0, 0]) == 2 and (counts("constant", 8) == 1).all()
    for K in (5, 1):      # every plane is the weight plane: p = 1 whatever the class; one class: the mask says 1
        mask_k = const if K == 5 else torch.ones_like(const)
        got = ops.scene_regions(mask_k, 8, canvas=weight.expand(K + 1, H, W).contiguous())
        assert got.label.tolist() == [0] and got.pixels.tolist() == [H * W] and got.bbox.tolist() == [[0, 0, W, H]]
        assert got.conf_sum.tolist() == [65536 * H * W] and got.conf_min.tolist() == [65536]
        assert got.sum_xy.tolist() == [[H * W * (W - 1) // 2, W * H * (H - 1) // 2]]

    # the checkerboard: 4096 labels in a full tile, more than the table takes, so the fallback runs (and is right: the
    # parametrised test compares all of it; here the region of every single pixel is spelled out)
    board = counts("checkerboard", 4)
    assert (board[full] == TILE * TILE).all() and (board[full] > TABLE).all()
    canvas, probs, weight_h = _canvas(H, W, 5)
    host = _mask("checkerboard", H, W)
    got = ops.scene_regions(torch.from_numpy(host.copy()).to(DEV), 4, canvas=canvas)
    q = rg.confidence(host, probs, weight_h).reshape(-1)
    idx = torch.arange(H * W, device=DEV)
    assert torch.equal(got.label.long(), idx) and (got.pixels == 1).all()
    assert torch.equal(got.sum_xy, torch.stack([idx % W, idx // W], dim=1)) and torch.equal(got.bbox[:, 2:] - got.bbox[:, :2], torch.ones_like(got.bbox[:, :2]))
    assert np.array_equal(got.conf_sum.cpu().numpy(), q) and np.array_equal(got.conf_min.cpu().numpy(), q)

    # the spiral: the arm is one region with pixels in every tile
    arm_labels = _labels("spiral", H, W, 4, None)[0]
    arm = _mask("spiral", H, W)
    assert arm[0, 0] == 1 and all((arm_labels[y:y + TILE, x:x + TILE] == 0).any() for y in range(0, H, TILE) for x in range(0, W, TILE))
    got = ops.scene_regions(torch.from_numpy(arm.copy()).to(DEV), 4)
    assert int(got.label[0]) == 0 and int(got.pixels[0]) == int(arm.sum()) and got.bbox[0].tolist() == [0, 0, W, H]

    # random-5 and percolation against the table's size: see the module's docstring
    for c, lo, hi in ((4, 2400, 2600), (8, 1450, 1600)):
        r5 = counts("random-5", c)
        assert ((r5[full] > lo) & (r5[full] < hi)).all() and (r5[full] > TABLE).all(), r5      # the table fills up: both paths in one workgroup
    rim = np.delete(counts("random-5", 4), full)[[0, 1, 2, 3, 4]]      # all but the 5 x 3 corner
    assert ((rim >= 100) & (rim <= TABLE // 4)).all(), rim      # hundreds: in use, nowhere near full
    perc = counts("percolation", 4)
    assert ((perc[full] >= 500) & (perc[full] <= TABLE * 3 // 5)).all(), perc      # hundreds in every full tile, never full


def test_other_argument_forms():
    H, W = 131, 197
    host = _mask("percolation", H, W)
    mask = torch.from_numpy(host.copy()).to(DEV)
    canvas, probs, weight = _canvas(H, W, 1)
    want = rg.regions(host, _labels("percolation", H, W, 8, None)[0], probs, weight)
    # a bool mask is the same mask
    got = ops.scene_regions(mask.bool(), 8, canvas=canvas)
    assert rg.same(_host(got), want) and got.value.dtype == torch.uint8
    # without a canvas the five other arrays are the same and the two confidences are None
    bare = ops.scene_regions(mask, 8)
    assert bare.conf_sum is None and bare.conf_min is None and _same(ops.SceneRegions(*got[:5], None, None), bare)
    # labels of the caller's: taken as they are (here: those of connectivity 4, whatever `connectivity` says)
    labels4 = ops.scene_components(mask, 4)[0]
    assert rg.same(_host(ops.scene_regions(mask, 8, canvas=canvas, labels=labels4)),
                   rg.regions(host, _labels("percolation", H, W, 4, None)[0], probs, weight))
    # every pixel ignored: no region, empty arrays of the right types, with and without a canvas
    for shape in ((H, W), (1, 1)):
        nothing = torch.full(shape, 3, dtype=torch.uint8, device=DEV)
        for cv in (None, torch.ones((6,) + shape, device=DEV)):
            empty = ops.scene_regions(nothing, 4, 3, canvas=cv)
            assert _check_form(empty, cv is not None) == 0
            ones = (None, None) if cv is None else (np.ones((5,) + shape, np.float32), np.ones(shape, np.float32))
            assert rg.same(_host(empty), rg.of_mask(nothing.cpu().numpy(), 4, 3, *ones))
    with pytest.raises(ValueError, match="scene_regions: the canvas is on cpu"):
        ops.scene_regions(mask, canvas=canvas.cpu())


# ------------------------------------------------------------------ 2. SceneInference.predict_features, DOFA, end to end
@pytest.fixture(scope="module", params=[5, 1], ids=["softmax5", "sigmoid1"])
def dofa(request, golden_dir):
    """The tiny DOFA recipe and the uint8 scene [3, 3 img, 2 img] of tests/test_hip_scene_sieve.py (values 1..255 with a block of
    zeros over rows 0 .. 1.5 img and columns 0 .. img)."""
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
    return nc, img, sm, scene


def _si(dofa, **kw) -> SceneInference:
    nc, img, sm, scene = dofa
    return SceneInference(sm, tile=(img, img), overlap=0.5, **{"batch_size": 64, "fill": 0, **kw})


SIEVE = 25      # pixels: the minimum mapping unit of the end-to-end cases


@pytest.mark.parametrize("kw,connectivity", [(dict(), 4), (dict(sieve=SIEVE), 4), (dict(sieve=SIEVE), 8),
                                             (dict(sieve=SIEVE, nodata=0, nodata_label=255), 4),
                                             (dict(sieve=SIEVE, nodata=0, nodata_label=7), 4)], ids=str)
def test_features_are_predict_rings_and_the_oracles_regions(dofa, kw, connectivity):
    nc, img, sm, scene = dofa
    si = _si(dofa, **kw)
    feats = si.predict_features(scene, connectivity=connectivity)
    assert isinstance(feats, SceneFeatures) and isinstance(feats.regions, ops.SceneRegions)
    plain = si.predict(scene, return_probs=True)
    assert torch.equal(feats.mask, plain.mask)
    vectors = si.predict_rings(scene, connectivity=connectivity)
    assert torch.equal(vectors.mask, feats.mask)
    for name, a, b in zip(feats.rings._fields, feats.rings, vectors.rings):
        assert torch.equal(a, b), name
    host, ignore = plain.mask.cpu().numpy(), kw.get("nodata_label", -1) if "nodata" in kw else -1
    if "nodata" in kw:
        assert (host[:3 * img // 2, :img] == ignore).all() and not (host[3 * img // 2:] == ignore).any()
    weight = si.canvas(scene)[nc].cpu().numpy()
    labels = so.components(host, connectivity, ignore)[0]
    want = rg.regions(host, labels, plain.probs.cpu().numpy(), weight)
    N = _check_form(feats.regions, True)
    assert N >= 2 and rg.same(_host(feats.regions), want)
    got = _host(feats.regions)
    assert (got.conf_min >= 0).all() and (got.conf_sum <= 65536 * got.pixels.astype(np.int64)).all() and (got.conf_sum > 0).any()

    if "sieve" in kw:      # a dissolved pixel counts with its new class's probability: some region's confidence is changed by it
        before = _si(dofa, **{**kw, "sieve": None}).predict(scene).mask.cpu().numpy()
        assert (before != host).any()
        q_before = rg.confidence(before, plain.probs.cpu().numpy(), weight)      # every pixel with the class the model gave it
        unsieved = np.zeros(N, dtype=np.int64)
        np.add.at(unsieved, np.searchsorted(got.label, labels[labels >= 0]), q_before[labels >= 0])
        changed = got.conf_sum != unsieved
        assert changed.any() and (got.conf_sum[changed] < unsieved[changed]).all()      # the new class was never the likelier one

    features = gscene.polygons(feats.rings, regions=feats.regions)
    assert len(features) == len(gscene.polygons(feats.rings)) == N
    assert all(0 <= f["properties"]["confidence_min"] <= f["properties"]["confidence"] <= 1 for f in features)
    assert [f["properties"]["label"] for f in features] == got.label.tolist()


def test_simplified_features_keep_their_regions(dofa):
    nc, img, sm, scene = dofa
    si = _si(dofa, sieve=SIEVE)
    exact, simple = si.predict_features(scene), si.predict_features(scene, simplify=1.5)
    assert torch.equal(exact.mask, simple.mask) and _same(exact.regions, simple.regions)
    want = si.predict_rings(scene, simplify=1.5).rings
    for name, a, b in zip(simple.rings._fields, simple.rings, want):
        assert torch.equal(a, b), name
    assert simple.rings.vertices.shape[0] < exact.rings.vertices.shape[0]
    features = gscene.polygons(simple.rings, regions=simple.regions)
    assert len(features) == len(gscene.polygons(simple.rings)) <= int(simple.regions.label.numel())
    assert all(0 <= f["properties"]["confidence"] <= 1 for f in features)
    # `values` selects rings, not regions
    some = si.predict_features(scene, values=[1])
    assert _same(some.regions, exact.regions) and set(some.rings.value.tolist()) == {1}
    assert {f["properties"]["value"] for f in gscene.polygons(some.rings, regions=some.regions)} == {1}
