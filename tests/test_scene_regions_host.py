"""Host side of the per-region attributes of whole-scene inference, no GPU: the binding of include/gdlhip_scene_regions.h
(SCENE_REGIONS_SIGNATURES) beside the other sets, the argument checks that fire before anything touches a device, the
``regions=`` keyword of ``gdlhip.scene.polygons`` on numpy inputs, and the numpy restatement the GPU tests compare with
(tests/_regions_oracle.py) held against results written out by hand and against ``scipy.ndimage``."""

import ctypes as C
import json

import numpy as np
import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
import _regions_oracle as rg  # noqa: E402
import _rings_oracle as ro  # noqa: E402
import _sieve_oracle as so  # noqa: E402
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402
from gdlhip import scene as gscene  # noqa: E402
from geo_deep_learning.tools import scene_inference as si  # noqa: E402

NAMES = ["gdl_scene_regions_count", "gdl_scene_regions_stats"]


# ------------------------------------------------------------------ the binding and the checks without a device
def test_regions_header_is_bound_beside_the_other_sets():
    i, p = C.c_int, C.c_void_p
    sig = _lib.SCENE_REGIONS_SIGNATURES
    assert sorted(sig) == NAMES
    assert sig["gdl_scene_regions_count"] == (i, [p, i, i, p, p, p, p])
    assert sig["gdl_scene_regions_stats"] == (i, [p, p, p, p, i, i, i, i, p, p, p, p, p, p, p, p])
    for other in (_lib.SIGNATURES, _lib.DEBUG_SIGNATURES, _lib.SCENE_SIGNATURES, _lib.SCENE_TTA_SIGNATURES, _lib.SCENE_NODATA_SIGNATURES,
                  _lib.SCENE_SIEVE_SIGNATURES, _lib.SCENE_RINGS_SIGNATURES, _lib.SCENE_SIMPLIFY_SIGNATURES):
        assert not set(sig) & set(other)
    assert not set(sig) & _lib.STATUS_FUNCTIONS and set(sig) <= _lib._CHECKED
    assert _lib.SCENE_REGIONS_SCAN_TILE == _lib.SCENE_SIMPLIFY_SCAN_TILE == 2048 and _lib.SCENE_REGIONS_TILE == 64
    table, probes = _lib.SCENE_REGIONS_TABLE, _lib.SCENE_REGIONS_PROBES
    assert table & (table - 1) == 0 and 1 <= probes <= table < 64 * 64      # a checkerboard tile cannot fit
    assert len(_lib.SCENE_SIMPLIFY_SIGNATURES) == 5 and len(_lib.SCENE_SIEVE_SIGNATURES) == 2      # the siblings keep their sizes


def test_regions_functions_are_exported_and_refuse_before_any_launch():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    raw, checked = _lib.load(), _lib.checked()
    for n, (res, args) in _lib.SCENE_REGIONS_SIGNATURES.items():
        assert getattr(raw, n).argtypes == args and getattr(raw, n).restype is res
        assert getattr(checked, n).errcheck is _lib.status_errcheck
    buf = (C.c_char * 64)()
    a = C.addressof(buf)      # never followed: every call below is refused first
    count = lambda H, W: raw.gdl_scene_regions_count(a, H, W, a, a, a, None)      # noqa: E731
    stats = lambda H, W, K, N, canvas=a: raw.gdl_scene_regions_stats(a, a, a, canvas, K, H, W, N, a, a, a, a, a, a, a, None)      # noqa: E731
    for name, call in (("gdl_scene_regions_count", count), ("gdl_scene_regions_stats", lambda H, W: stats(H, W, 5, 1))):
        for H, W in ((65536, 32768), (2, 2 ** 30), (46341, 46341)):      # H * W >= 2^31
            assert call(H, W) == -1
            assert f"{name}: {H} x {W} pixels".encode() in raw.gdl_last_error() and b"2^31" in raw.gdl_last_error()
        for H, W in ((0, 4), (4, 0), (-1, 4)):
            assert call(H, W) == -1 and f"{name}: bad sizes".encode() in raw.gdl_last_error()
    assert raw.gdl_scene_regions_count(a, 4, 4, None, a, a, None) == -1 and b"gdl_scene_regions_count: null pointer" in raw.gdl_last_error()
    assert raw.gdl_scene_regions_count(a, 4, 4, a, a, None, None) == -1 and b"gdl_scene_regions_count: null pointer" in raw.gdl_last_error()
    for K in (0, 256, -1):
        assert stats(4, 4, K, 1) == -1 and f"gdl_scene_regions_stats: 1..255 classes, got {K}".encode() in raw.gdl_last_error()
    for N in (-1, 17):
        assert stats(4, 4, 5, N) == -1 and f"gdl_scene_regions_stats: {N} regions in 4 x 4 pixels".encode() in raw.gdl_last_error()
    assert raw.gdl_scene_regions_stats(a, a, None, a, 5, 4, 4, 1, a, a, a, a, a, a, a, None) == -1 and b"null pointer" in raw.gdl_last_error()
    # with a canvas the two confidence arrays are needed, without one they are not looked at (and K is not either)
    assert raw.gdl_scene_regions_stats(a, a, a, a, 5, 4, 4, 1, a, a, a, a, a, None, a, None) == -1 and b"null pointer" in raw.gdl_last_error()
    assert raw.gdl_scene_regions_stats(a, a, a, a, 5, 4, 4, 1, a, a, a, a, a, a, None, None) == -1 and b"null pointer" in raw.gdl_last_error()
    # no region: nothing is launched and nothing is asked of the pointers
    assert raw.gdl_scene_regions_stats(None, None, None, None, 0, 4, 4, 0, None, None, None, None, None, None, None, None) == 0
    with pytest.raises(ValueError, match="gdl_scene_regions_stats: 1..255 classes, got 256"):
        checked.gdl_scene_regions_stats(a, a, a, a, 256, 4, 4, 1, a, a, a, a, a, a, a, None)


def test_ops_scene_regions_checks_its_arguments_before_a_device_is_needed():
    mask = torch.zeros((5, 7), dtype=torch.uint8)
    labels, canvas = torch.zeros((5, 7), dtype=torch.int32), torch.ones((6, 5, 7))
    op = "scene_regions"
    with pytest.raises(ValueError, match="device tensors"):      # every argument is fine: the device is asked for last
        ops.scene_regions(mask, 8, 3, canvas=canvas, labels=labels)
    with pytest.raises(ValueError, match="device tensors"):
        ops.scene_regions(mask.bool())
    with pytest.raises(ValueError, match=f"{op}: contiguous uint8 / bool \\[H, W\\] mask expected, got torch.int64"):
        ops.scene_regions(mask.long())
    with pytest.raises(ValueError, match=f"{op}: contiguous uint8 / bool"):
        ops.scene_regions(mask.t())
    with pytest.raises(ValueError, match=f"{op}: connectivity must be 4 or 8, got 6"):
        ops.scene_regions(mask, connectivity=6)
    for bad in (-1, 256, 1.0, True):
        with pytest.raises(ValueError, match=f"{op}: ignore_label must be None or an int in 0..255"):
            ops.scene_regions(mask, ignore_label=bad)
    with pytest.raises(ValueError, match=f"{op}: empty mask"):
        ops.scene_regions(torch.zeros((0, 7), dtype=torch.uint8))
    for bad in (labels.long(), labels[:4], labels.t().contiguous().t(), labels.numpy(), labels.reshape(-1)):
        with pytest.raises(ValueError, match=f"{op}: labels must be a contiguous int32 \\[H, W\\] = \\[5, 7\\] tensor"):
            ops.scene_regions(mask, labels=bad)
    for bad in (canvas.double(), canvas[0], canvas[:, :4], canvas[:1], torch.ones((257, 5, 7)), canvas.permute(0, 2, 1).contiguous().permute(0, 2, 1),
                canvas.numpy()):
        with pytest.raises(ValueError, match=f"{op}: canvas must be a contiguous f32 \\[K \\+ 1, H, W\\]"):
            ops.scene_regions(mask, canvas=bad)
    assert ops.SceneRegions._fields == ("label", "value", "pixels", "bbox", "sum_xy", "conf_sum", "conf_min") == rg.Regions._fields
    assert si.SceneFeatures._fields == ("mask", "rings", "regions") and si.SceneVectors._fields == ("mask", "rings")
    sm = si.ScriptModel(torch.nn.Identity(), device=torch.device("cpu"), num_classes=2, input_shape=(1, 3, 16, 16))
    for bad in (-1.0, float("nan"), 2 ** 20 + 1, "1", True):
        with pytest.raises(ValueError, match="SceneInference.predict_features: simplify must be None or a finite tolerance"):
            si.SceneInference(sm, tile=(16, 16)).predict_features(torch.zeros((3, 16, 16), dtype=torch.uint8), simplify=bad)


# ------------------------------------------------------------------ the oracle, by hand and against scipy
@pytest.mark.parametrize("name,mask,kw,probs,weight,want", rg.HAND_CASES, ids=[c[0] for c in rg.HAND_CASES])
def test_the_oracle_on_hand_drawn_cases(name, mask, kw, probs, weight, want):
    before = mask.copy()
    got = rg.of_mask(mask, probs=probs, weight=weight, **kw)
    assert rg.same(got, want), f"\n{got}\n{want}"
    assert np.array_equal(mask, before)
    assert int(got.pixels.sum()) == int((mask != kw.get("ignore_label", -1)).sum())


def test_the_hand_cases_cover_what_they_are_for():
    names = " / ".join(c[0] for c in rg.HAND_CASES)
    for what in ("hole", "connectivity 4", "connectivity 8", "ignored stripe", "K = 1", "uncovered", "no plane"):
        assert what in names, what
    one = [c for c in rg.HAND_CASES if "both values" in c[0]][0]
    assert one[3].shape[0] == 1 and set(one[1].ravel()) == {0, 1} and (one[4] == 0).sum() == 1
    assert any(c[3] is None for c in rg.HAND_CASES)


def _canvas_like(H: int, W: int, K: int, seed: int):
    """f32 probabilities [K, H, W] and a weight plane with a block of zeros, as a finished canvas would give them."""
    g = np.random.default_rng([seed, H, W, K])
    weight = g.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    weight[H // 3:H // 3 + 5, W // 4:W // 4 + 9] = 0
    raw = g.uniform(0.01, 1.0, (max(K, 2), H, W)).astype(np.float32)
    probs = (raw / raw.sum(axis=0, dtype=np.float32))[:K].astype(np.float32)
    return np.where(weight != 0, probs, np.float32(0)).astype(np.float32), weight


@pytest.mark.parametrize("name", list(so.patterns(16)))
def test_the_oracle_agrees_with_scipy(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    make, ignore = so.patterns(16)[name]
    for H, W in ((70, 45), (37, 53), (1, 40), (40, 1), (1, 1)):
        mask = make(H, W)
        for K in (5, 1):
            probs, weight = _canvas_like(H, W, K, 11)
            q = rg.confidence(mask, probs, weight)
            assert q.dtype == np.int32 and q.min() >= 0 and q.max() <= 65536
            for connectivity, ign in ((4, -1), (8, ignore)):
                labels = so.components(mask, connectivity, ign)[0]
                got = rg.regions(mask, labels, probs, weight)
                N = len(got.label)
                assert np.array_equal(got.label, np.unique(labels[labels >= 0])) and np.array_equal(got.value, mask.reshape(-1)[got.label])
                if N == 0:
                    assert (mask == ign).all()
                    continue
                zones = np.where(labels >= 0, np.searchsorted(got.label, labels) + 1, 0)      # scipy: 0 is the background
                index = np.arange(1, N + 1)
                where = (name, H, W, K, connectivity, ign)
                assert np.array_equal(got.pixels, ndimage.sum(np.ones((H, W)), zones, index).astype(np.int64)), where
                assert np.array_equal(got.conf_sum, ndimage.sum(q.astype(np.float64), zones, index).astype(np.int64)), where
                assert np.array_equal(got.conf_min, ndimage.minimum(q, zones, index)), where
                boxes = [(sx.start, sy.start, sx.stop, sy.stop) for sy, sx in ndimage.find_objects(zones, max_label=N)]
                assert np.array_equal(got.bbox, np.array(boxes)), where
                centre = np.array(ndimage.center_of_mass(np.ones((H, W)), zones, index))      # (y, x) of the pixel indices
                assert np.allclose(got.sum_xy / got.pixels[:, None], centre[:, ::-1], rtol=0, atol=1e-9), where


def test_the_confidence_rules_one_by_one():
    mask = np.array([[0, 1, 2, 3, 0, 1]], dtype=np.uint8)
    weight = np.array([[1, 1, 1, 1, 0, 0]], dtype=np.float32)
    p3 = np.array([[[0.25] * 6], [[0.5] * 6], [[0.125] * 6]], dtype=np.float32)
    assert rg.confidence(mask, p3, weight).tolist() == [[16384, 32768, 8192, 0, 0, 0]]
    p1 = np.array([[[0.25, 0.25, 0.25, 0.25, 0.0, 0.0]]], dtype=np.float32)
    assert rg.confidence(mask, p1, weight).tolist() == [[49152, 16384, 0, 0, 0, 0]]
    # ties go to even, as rintf rounds: 0.5 / 65536 and 1.5 / 65536 are exact in f32
    half = np.array([[[0.5 / 65536, 1.5 / 65536, 2.5 / 65536]]], dtype=np.float32)
    assert rg.confidence(np.ones((1, 3), dtype=np.uint8), half, np.ones((1, 3), dtype=np.float32)).tolist() == [[0, 2, 2]]


# ------------------------------------------------------------------ polygons(..., regions=)
def _mask_with_a_hole() -> np.ndarray:
    m = so._rows("0000000", "0111110", "0100010", "0102010", "0100010", "0111110")
    return m


def _host(mask: np.ndarray, probs=None, weight=None, **kw):
    return ro.trace(mask, **kw), rg.of_mask(mask, probs=probs, weight=weight, **kw)


def test_polygons_gain_the_regions_attributes():
    mask = _mask_with_a_hole()
    H, W = mask.shape
    probs, weight = _canvas_like(H, W, 3, 5)
    rings, regions = _host(mask, probs, weight)
    plain = gscene.polygons(rings)
    feats = gscene.polygons(rings, regions=regions)
    assert len(feats) == len(plain) == len(regions.label) == 4
    q = rg.confidence(mask, probs, weight)
    labels = so.components(mask, 4)[0]
    for f, p in zip(feats, plain):
        props = f["properties"]
        assert list(props) == ["value", "label", "pixels", "bbox", "centroid", "confidence", "confidence_min"]
        assert f["geometry"] == p["geometry"] and {k: props[k] for k in p["properties"]} == p["properties"]
        ys, xs = np.nonzero(labels == props["label"])
        assert props["pixels"] == len(xs)
        assert props["bbox"] == [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1] and all(type(v) is int for v in props["bbox"])
        assert props["centroid"] == pytest.approx([xs.mean() + 0.5, ys.mean() + 0.5], abs=1e-12)
        mine = q[labels == props["label"]]
        assert props["confidence"] == pytest.approx(mine.mean() / 65536, abs=1e-12) and 0 <= props["confidence"] <= 1
        assert props["confidence_min"] == mine.min() / 65536
    ring = [f for f in feats if f["properties"]["value"] == 1][0]["properties"]
    assert ring["bbox"] == [1, 1, 6, 6] and ring["centroid"] == [3.5, 3.5] and ring["pixels"] == 16
    json.dumps(feats)      # plain Python numbers throughout
    # tensors are taken as arrays are
    as_tensors = ops.SceneRegions(*(torch.from_numpy(f.copy()) for f in regions))
    assert gscene.polygons(ops.SceneRings(*(torch.from_numpy(f.copy()) for f in rings)), regions=as_tensors) == feats


def test_polygons_without_confidences_and_with_a_transform():
    mask = _mask_with_a_hole()
    rings, regions = _host(mask)
    assert regions.conf_sum is None and regions.conf_min is None
    feats = gscene.polygons(rings, regions=regions)
    assert all(list(f["properties"]) == ["value", "label", "pixels", "bbox", "centroid"] for f in feats)
    t = (10.0, 0.5, 500000.0, 0.25, -10.0, 4000000.0)
    moved = gscene.polygons(rings, transform=t, regions=regions)
    for f, g in zip(feats, moved):
        cx, cy = f["properties"]["centroid"]
        assert g["properties"]["centroid"] == [10.0 * cx + 0.5 * cy + 500000.0, 0.25 * cx - 10.0 * cy + 4000000.0]
        assert g["properties"]["bbox"] == f["properties"]["bbox"]      # pixel indices stay pixel indices
    assert [g["geometry"] for g in moved] == [g["geometry"] for g in gscene.polygons(rings, transform=t)]


def test_polygons_without_regions_are_byte_for_byte_what_they_were():
    for name in ("random-5", "rings", "ignore-cross"):
        make, ignore = so.patterns(16)[name]
        mask = make(37, 53)
        rings = ro.trace(mask, connectivity=8, ignore_label=ignore)
        for transform in (None, (2.0, 0.0, 100.0, 0.0, -2.0, 900.0)):
            a, b = gscene.polygons(rings, transform), gscene.polygons(rings, transform, regions=None)
            assert json.dumps(a) == json.dumps(b) and a == b
            assert all(list(f["properties"]) == ["value", "label", "pixels"] for f in a)
            both = gscene.polygons(rings, transform, regions=rg.of_mask(mask, 8, ignore))
            assert [f["geometry"] for f in both] == [f["geometry"] for f in a]


def test_polygons_refuse_regions_of_another_mask():
    mask = _mask_with_a_hole()
    rings, regions = _host(mask)
    k = 2
    missing = rg.Regions(*(None if f is None else np.delete(f, k, axis=0) for f in regions))
    with pytest.raises(ValueError, match=f"polygons: the rings have label {int(regions.label[k])}, the regions do not"):
        gscene.polygons(rings, regions=missing)
    pixels = regions.pixels.copy()
    pixels[1] += 1
    with pytest.raises(ValueError, match=f"polygons: label {int(regions.label[1])} has {int(regions.pixels[1])} pixels by its rings and "
                                         f"{int(pixels[1])} by the regions"):
        gscene.polygons(rings, regions=regions._replace(pixels=pixels))
    with pytest.raises(ValueError, match="polygons: the fields of regions do not belong together"):
        gscene.polygons(rings, regions=regions._replace(bbox=regions.bbox[:-1]))
    # regions the rings do not have are passed over: rings of one class alone
    ones = ro.trace(mask, values=[1])
    feats = gscene.polygons(ones, regions=regions)
    assert len(feats) == 1 and feats[0]["properties"]["value"] == 1 and feats[0]["properties"]["bbox"] == [1, 1, 6, 6]


def test_a_feature_dropped_for_its_collapsed_exterior_stays_dropped():
    mask = _mask_with_a_hole()
    rings, regions = _host(mask)
    r = int(np.nonzero(rings.value == 2)[0][0])      # the single pixel of class 2: its ring collapses to two vertices
    lo, hi = int(rings.ring_offsets[r]), int(rings.ring_offsets[r + 1])
    vertices = np.delete(rings.vertices, range(lo + 2, hi), axis=0)
    offsets = rings.ring_offsets.copy()
    offsets[r + 1:] -= hi - lo - 2
    collapsed = rings._replace(vertices=vertices, ring_offsets=offsets)
    a, b = gscene.polygons(collapsed), gscene.polygons(collapsed, regions=regions)
    assert len(a) == len(b) == 3 and [f["properties"]["label"] for f in a] == [f["properties"]["label"] for f in b]
    assert 2 not in [f["properties"]["value"] for f in b]
