"""Host side of the polygon rings of whole-scene inference, no GPU: the binding of include/gdlhip_scene_rings.h
(SCENE_RINGS_SIGNATURES) and the argument checks that fire before anything touches a device, the sequential tracer the GPU tests
compare with (tests/_rings_oracle.py) held against its own inverse, against ``scipy.ndimage.label`` and against rings written out
vertex by vertex, and ``gdlhip.scene.polygons``.

One property is stated more narrowly than "under connectivity 4 no ring repeats a lattice point": a 4-connected region can touch
itself across a diagonal (two of its pixels NW and SE of a lattice point, other values NE and SW), and when both passes lie on
one ring -- the background around two diagonal blocks, say -- that ring visits the point twice whatever the tracer.  What holds,
and is tested, is that a ring repeats a lattice point only at such a pinch of its own value, at most twice, and that it turns
towards its own pixel (clockwise) there under connectivity 4 and away from it under connectivity 8."""

import ctypes as C
import functools
from collections import Counter

import numpy as np
import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
import _rings_oracle as ro  # noqa: E402
import _sieve_oracle as so  # noqa: E402
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402
from gdlhip import scene as gscene  # noqa: E402
from geo_deep_learning.tools.scene_inference import SceneInference, SceneVectors  # noqa: E402

NAMES = ["gdl_scene_rings_count", "gdl_scene_rings_trace", "gdl_scene_rings_write"]
PATTERNS = so.patterns(64)
SHAPES = [(37, 53), (131, 197)]


# ------------------------------------------------------------------ the binding and the checks without a device
def test_rings_header_is_bound_beside_the_other_sets():
    i, p = C.c_int, C.c_void_p
    sig = _lib.SCENE_RINGS_SIGNATURES
    assert sorted(sig) == NAMES
    assert sig["gdl_scene_rings_count"] == (i, [p, i, i, i, p, p, p, p, p])
    assert sig["gdl_scene_rings_trace"] == (i, [p, i, i, i, i, p, p, i, p, p, p, p, p, p, p])
    assert sig["gdl_scene_rings_write"] == (i, [p, p, i, i, i, i, p, p, p, p, p, p, p, p, p, p, p, p])
    for other in (_lib.SIGNATURES, _lib.DEBUG_SIGNATURES, _lib.SCENE_SIGNATURES, _lib.SCENE_TTA_SIGNATURES, _lib.SCENE_NODATA_SIGNATURES,
                  _lib.SCENE_SIEVE_SIGNATURES):
        assert not set(sig) & set(other)
    assert not set(sig) & _lib.STATUS_FUNCTIONS and set(sig) <= _lib._CHECKED
    assert (_lib.SCENE_RINGS_SCAN_TILE, _lib.SCENE_RINGS_FLAGS) == (2048, 64)
    assert len(_lib.SCENE_SIEVE_SIGNATURES) == 2      # the sieve's set keeps its size


def test_rings_functions_are_exported_and_refuse_before_any_launch():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    raw, checked = _lib.load(), _lib.checked()
    for n, (res, args) in _lib.SCENE_RINGS_SIGNATURES.items():
        assert getattr(raw, n).argtypes == args and getattr(raw, n).restype is res
        assert getattr(checked, n).errcheck is _lib.status_errcheck
    buf = (C.c_char * 64)()
    a = C.addressof(buf)      # never followed: every call below is refused first
    count = lambda H, W, ign: raw.gdl_scene_rings_count(a, H, W, ign, a, a, a, a, None)      # noqa: E731
    trace = lambda H, W, conn, ign, E=4: raw.gdl_scene_rings_trace(a, H, W, conn, ign, a, a, E, a, a, a, a, a, a, None)      # noqa: E731
    assert raw.gdl_scene_rings_count(a, 4, 4, -1, a, None, a, a, None) == -1 and b"gdl_scene_rings_count: null pointer" in raw.gdl_last_error()
    assert raw.gdl_scene_rings_trace(a, 4, 4, 4, -1, a, a, 4, a, a, None, a, a, a, None) == -1
    assert b"gdl_scene_rings_trace: null pointer" in raw.gdl_last_error()
    assert raw.gdl_scene_rings_write(a, a, 4, 4, 1, 4, a, a, a, a, a, a, a, a, a, a, None, None) == -1
    assert b"gdl_scene_rings_write: null pointer" in raw.gdl_last_error()
    for H, W in ((32768, 16384), (2, 2 ** 28), (23171, 23171)):      # H * W >= 2^29: a slot would not fit an int32
        assert H * W >= 2 ** 29
        for name, call in (("gdl_scene_rings_count", lambda: count(H, W, -1)), ("gdl_scene_rings_trace", lambda: trace(H, W, 4, -1))):
            assert call() == -1 and f"{name}: {H} x {W} pixels".encode() in raw.gdl_last_error() and b"2^29" in raw.gdl_last_error()
    for H, W in ((0, 4), (4, 0), (-1, 4)):
        assert count(H, W, -1) == -1 and b"gdl_scene_rings_count: bad sizes" in raw.gdl_last_error()
        assert trace(H, W, 4, -1) == -1 and b"gdl_scene_rings_trace: bad sizes" in raw.gdl_last_error()
    for ign in (-2, 256):
        assert count(4, 4, ign) == -1 and f"gdl_scene_rings_count: ignore_label {ign} is not in -1..255".encode() in raw.gdl_last_error()
        assert trace(4, 4, 4, ign) == -1
    for conn in (6, 0, 5):
        assert trace(4, 4, conn, -1) == -1 and f"gdl_scene_rings_trace: connectivity {conn} is neither 4 nor 8".encode() in raw.gdl_last_error()
    for E in (-1, 65):      # more sides than 4 * H * W
        assert trace(4, 4, 4, -1, E) == -1 and f"gdl_scene_rings_trace: n_sides {E}".encode() in raw.gdl_last_error()
    for E, R, V in ((4, 0, 0), (0, 1, 4), (8, 2, 7), (3, 1, 4), (4, 1, 0), (4, -1, 4)):      # counts no mask can give
        assert raw.gdl_scene_rings_write(a, a, 4, E, R, V, a, a, a, a, a, a, a, a, a, a, a, None) == -1, (E, R, V)
    with pytest.raises(ValueError, match="gdl_scene_rings_trace: connectivity 6"):
        checked.gdl_scene_rings_trace(a, 4, 4, 6, -1, a, a, 4, a, a, a, a, a, a, None)


def test_ops_and_predict_rings_check_their_arguments_before_the_device():
    mask = torch.zeros((5, 7), dtype=torch.uint8)
    for bad in (dict(connectivity=6), dict(values=[256]), dict(values=[-1]), dict(values=[1.5]), dict(values=7), dict(values="1"),
                dict(values=[False]), dict(ignore_label=300), dict(labels=torch.zeros((7, 5), dtype=torch.int32)),
                dict(labels=torch.zeros((5, 7), dtype=torch.int64)), dict(labels=np.zeros((5, 7), dtype=np.int32))):
        with pytest.raises(ValueError, match="scene_rings: "):
            ops.scene_rings(mask, **bad)
    with pytest.raises(ValueError, match="scene_rings: .*mask expected"):
        ops.scene_rings(mask.float())
    with pytest.raises(ValueError, match="device tensors"):      # every other argument is fine: the device is asked for last
        ops.scene_rings(mask, 8, 3, values=range(4), labels=torch.zeros((5, 7), dtype=torch.int32))
    assert ops._keep_table(None) == [1] * 256 and sum(ops._keep_table([])) == 0
    assert [v for v, k in enumerate(ops._keep_table(iter((3, 1, 3)))) if k] == [1, 3]
    assert tuple(ops.SceneRings._fields) == ("vertices", "ring_offsets", "value", "label", "start", "area2")
    assert tuple(SceneVectors._fields) == ("mask", "rings") and callable(SceneInference.predict_rings)


# ------------------------------------------------------------------ the tracer on the patterns
@functools.lru_cache(maxsize=None)
def _case(name: str, H: int, W: int, connectivity: int, ignore: int):
    mask = PATTERNS[name][0](H, W)
    labels, sizes = so.components(mask, connectivity, ignore)
    return mask, labels, sizes, ro.trace(mask, connectivity, ignore, labels=labels)


def _cases():
    return [(name, H, W, c, ign) for name in PATTERNS for H, W in SHAPES for c in (4, 8) for ign in (-1, PATTERNS[name][1])]


def _ring(rings: ro.Rings, r: int) -> np.ndarray:
    return rings.vertices[rings.ring_offsets[r]:rings.ring_offsets[r + 1]].astype(np.int64)


@pytest.mark.parametrize("name,H,W,connectivity,ignore", _cases(), ids=lambda v: str(v))
def test_the_successor_map_is_a_permutation_and_its_cycles_are_the_rings(name, H, W, connectivity, ignore):
    mask, labels, sizes, rings = _case(name, H, W, connectivity, ignore)
    boundary, nxt = ro.successor(mask, connectivity, ignore)
    sides = np.flatnonzero(boundary)
    assert (nxt[~boundary] == -1).all() and boundary[nxt[sides]].all(), "a boundary side leads to a boundary side"
    assert np.array_equal(np.sort(nxt[sides]), sides), "and every boundary side is led to once"
    assert (labels.reshape(-1)[nxt[sides] >> 2] == labels.reshape(-1)[sides >> 2]).all(), "a ring stays in its component"
    # every slot lies in exactly one ring: the rings' side counts add up to the boundary sides, and the tracer marks none twice
    lengths = [int(np.abs(np.roll(v, -1, axis=0) - v).sum()) for v in (_ring(rings, r) for r in range(len(rings.value)))]
    assert sum(lengths) == len(sides)
    assert (np.diff(rings.start) > 0).all() and boundary[rings.start].all(), "rings by ascending start"
    assert np.array_equal(rings.value, mask.reshape(-1)[rings.start >> 2]) and np.array_equal(rings.label, labels.reshape(-1)[rings.start >> 2])


@pytest.mark.parametrize("name,H,W,connectivity,ignore", _cases(), ids=lambda v: str(v))
def test_the_rings_are_canonical_and_fill_back_to_the_components(name, H, W, connectivity, ignore):
    mask, labels, sizes, rings = _case(name, H, W, connectivity, ignore)
    assert np.array_equal(ro.fill(rings, H, W), labels), "fill reproduces labels == label for every component"
    present = np.flatnonzero(sizes)
    exterior = rings.area2 > 0
    assert (rings.area2 != 0).all()
    assert np.array_equal(np.sort(rings.label[exterior]), present), "one exterior ring per component"
    assert np.array_equal(rings.start[exterior], 4 * rings.label[exterior]), "and it starts at the top side of the component's first pixel"
    total = np.zeros(H * W, dtype=np.int64)
    np.add.at(total, rings.label, rings.area2)
    assert np.array_equal(total, 2 * sizes.astype(np.int64)), "the area2 of a component's rings add up to twice its size"
    value = int(rings.value[0]) if len(rings.value) else -1
    for r in range(len(rings.value)):
        v = _ring(rings, r)
        step, turn = np.roll(v, -1, axis=0) - v, None
        assert len(v) >= 4 and ((step != 0).sum(axis=1) == 1).all(), "segments along the axes, none of length 0"
        assert ((step * np.roll(step, -1, axis=0)).sum(axis=1) == 0).all(), "consecutive segments are perpendicular"
        if len(set(map(tuple, v.tolist()))) == len(v):
            continue
        # a repeated lattice point: a pinch of the ring's own value, visited twice, turning towards the region (clockwise with y
        # down: a positive cross product) under connectivity 4 and away from it under connectivity 8
        value = int(rings.value[r])
        turn = np.roll(step, 1, axis=0)[:, 0] * step[:, 1] - np.roll(step, 1, axis=0)[:, 1] * step[:, 0]      # at v[k]: step in x step out
        for (x, y), n in Counter(map(tuple, v.tolist())).items():
            if n == 1:
                continue
            assert n == 2 and 0 < x < W and 0 < y < H
            nw, ne, sw, se = (int(mask[y - 1, x - 1]) == value, int(mask[y - 1, x]) == value, int(mask[y, x - 1]) == value,
                              int(mask[y, x]) == value)
            assert (nw, ne, sw, se) in ((True, False, False, True), (False, True, True, False)), "a pinch of the ring's value"
            at = turn[(v[:, 0] == x) & (v[:, 1] == y)]
            assert (at > 0).all() if connectivity == 4 else (at < 0).all()


@pytest.mark.parametrize("name", list(PATTERNS))
def test_exterior_rings_are_counted_as_scipy_counts_components(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    for H, W in SHAPES:
        for connectivity in (4, 8):
            mask, labels, sizes, rings = _case(name, H, W, connectivity, -1)
            structure = None if connectivity == 4 else np.ones((3, 3), dtype=int)
            for value in np.unique(mask).tolist():
                want = ndimage.label(mask == value, structure)[1]
                assert int(((rings.value == value) & (rings.area2 > 0)).sum()) == want, (H, W, connectivity, value)


def test_the_keep_set_drops_rings_and_changes_no_other():
    mask, labels, sizes, rings = _case("random-5", 37, 53, 8, -1)
    kept = ro.trace(mask, 8, -1, (1, 3), labels)
    pick = np.isin(rings.value, (1, 3))
    assert pick.any() and not pick.all()
    for field in ("value", "label", "start", "area2"):
        assert np.array_equal(getattr(kept, field), getattr(rings, field)[pick]), field
    assert np.array_equal(kept.vertices, np.concatenate([_ring(rings, r) for r in np.flatnonzero(pick)]))
    assert np.array_equal(ro.fill(kept, 37, 53), np.where(np.isin(mask, (1, 3)), labels, -1))
    assert len(ro.trace(mask, 8, -1, ()).value) == 0 and ro.trace(mask, 8, -1, ()).ring_offsets.tolist() == [0]


# ------------------------------------------------------------------ rings written out by hand, 5 x 7
def _rows(*rows: str) -> np.ndarray:
    return np.array([[int(c) for c in r] for r in rows], dtype=np.uint8)


DIAGONAL = so.HAND_CASES[6][1]      # "1100000", "1100000", "0011000", "0011000", "0000000"
PIXEL_AND_BLOCK = _rows("0000000", "0100000", "0011000", "0011000", "0000000")
FENCED = so.HAND_CASES[2][1]        # "0000001", "0099900", "0092900", "0099900", "0000000"
OUTLINE = [(7, 0), (7, 5), (0, 5), (0, 0)]      # of the whole raster
# (name, mask, keyword arguments, [(value, label, start, area2, vertices)])
HAND_RINGS = [
    ("a single pixel", _rows("0000000", "0000000", "0001000", "0000000", "0000000"), dict(values=[1]),
     [(1, 17, 68, 2, [(4, 2), (4, 3), (3, 3), (3, 2)])]),
    ("a single pixel and the background around it: the same square the other way round",
     _rows("0000000", "0000000", "0001000", "0000000", "0000000"), dict(),
     [(0, 0, 0, 70, OUTLINE), (0, 0, 42, -2, [(3, 2), (3, 3), (4, 3), (4, 2)]), (1, 17, 68, 2, [(4, 2), (4, 3), (3, 3), (3, 2)])]),
    ("a 3 x 3 block with a centre hole", _rows("0000000", "0011100", "0010100", "0011100", "0000000"), dict(values=[1]),
     [(1, 9, 36, 18, [(5, 1), (5, 4), (2, 4), (2, 1)]), (1, 9, 42, -2, [(3, 2), (3, 3), (4, 3), (4, 2)])]),
    # the first block fills the raster's corner, so the background's exterior runs round it, and on round the second block, which
    # the background reaches round only through the shared point (2, 2): one ring that touches (2, 2) twice, and no hole
    ("two blocks across a diagonal, connectivity 4: two squares", DIAGONAL, dict(connectivity=4),
     [(1, 0, 0, 8, [(2, 0), (2, 2), (0, 2), (0, 0)]),
      (0, 2, 8, 54, [(7, 0), (7, 5), (0, 5), (0, 2), (2, 2), (2, 4), (4, 4), (4, 2), (2, 2), (2, 0)]),
      (1, 16, 64, 8, [(4, 2), (4, 4), (2, 4), (2, 2)])]),
    ("two blocks across a diagonal, connectivity 8: one exterior of 8 vertices through the shared point twice", DIAGONAL, dict(connectivity=8),
     [(1, 0, 0, 16, [(2, 0), (2, 2), (4, 2), (4, 4), (2, 4), (2, 2), (0, 2), (0, 0)]),
      (0, 2, 8, 62, [(7, 0), (7, 5), (0, 5), (0, 2), (2, 2), (2, 0)]),
      (0, 2, 38, -8, [(2, 2), (2, 4), (4, 4), (4, 2)])]),
    ("a pixel and a block across a diagonal, connectivity 4: two exteriors, and one hole of the background round both",
     PIXEL_AND_BLOCK, dict(connectivity=4),
     [(0, 0, 0, 70, OUTLINE), (0, 0, 6, -10, [(1, 1), (1, 2), (2, 2), (2, 4), (4, 4), (4, 2), (2, 2), (2, 1)]),
      (1, 8, 32, 2, [(2, 1), (2, 2), (1, 2), (1, 1)]), (1, 16, 64, 8, [(4, 2), (4, 4), (2, 4), (2, 2)])]),
    ("a pixel and a block across a diagonal, connectivity 8: one exterior, and the background has two holes",
     PIXEL_AND_BLOCK, dict(connectivity=8),
     [(0, 0, 0, 70, OUTLINE), (0, 0, 6, -2, [(1, 1), (1, 2), (2, 2), (2, 1)]),
      (1, 8, 32, 10, [(2, 1), (2, 2), (4, 2), (4, 4), (2, 4), (2, 2), (1, 2), (1, 1)]), (0, 0, 38, -8, [(2, 2), (2, 4), (4, 4), (4, 2)])]),
    ("a keep set that drops the background", DIAGONAL, dict(connectivity=4, values=[1]),
     [(1, 0, 0, 8, [(2, 0), (2, 2), (0, 2), (0, 0)]), (1, 16, 64, 8, [(4, 2), (4, 4), (2, 4), (2, 2)])]),
    ("fenced in by ignore_label 9: the fence has no ring, what it fences has", FENCED, dict(ignore_label=9),
     [(0, 0, 0, 68, [(6, 0), (6, 1), (7, 1), (7, 5), (0, 5), (0, 0)]), (0, 0, 10, -18, [(2, 1), (2, 4), (5, 4), (5, 1)]),
      (1, 6, 24, 2, [(7, 0), (7, 1), (6, 1), (6, 0)]), (2, 17, 68, 2, [(4, 2), (4, 3), (3, 3), (3, 2)])]),
]


def _as_rings(rows) -> ro.Rings:
    vertices = [xy for row in rows for xy in row[4]]
    return ro.Rings(np.array(vertices, dtype=np.int32).reshape(-1, 2), np.cumsum([0] + [len(row[4]) for row in rows]).astype(np.int32),
                    np.array([row[0] for row in rows], dtype=np.uint8), np.array([row[1] for row in rows], dtype=np.int32),
                    np.array([row[2] for row in rows], dtype=np.int32), np.array([row[3] for row in rows], dtype=np.int64))


@pytest.mark.parametrize("name,mask,kw,rows", HAND_RINGS, ids=[c[0] for c in HAND_RINGS])
def test_the_tracer_on_the_hand_drawn_cases(name, mask, kw, rows):
    got, want = ro.trace(mask, **kw), _as_rings(rows)
    for field in want._fields:
        assert np.array_equal(getattr(got, field), getattr(want, field)), f"{field}\n{getattr(got, field)}"
        assert getattr(got, field).dtype == getattr(want, field).dtype


# ------------------------------------------------------------------ polygons
def test_polygons_group_close_and_order():
    rings = _as_rings(HAND_RINGS[6][3])      # the pixel and the block, connectivity 8: labels 0 (two holes) and 8
    features = gscene.polygons(rings)
    assert [f["type"] for f in features] == ["Feature", "Feature"] and all(f["geometry"]["type"] == "Polygon" for f in features)
    assert [f["properties"] for f in features] == [{"value": 0, "label": 0, "pixels": 30}, {"value": 1, "label": 8, "pixels": 5}]
    ground, blob = (f["geometry"]["coordinates"] for f in features)
    assert ground == [[[7, 0], [7, 5], [0, 5], [0, 0], [7, 0]],      # the exterior first, closed
                      [[1, 1], [1, 2], [2, 2], [2, 1], [1, 1]],      # then the holes by ascending start: 6 before 38
                      [[2, 2], [2, 4], [4, 4], [4, 2], [2, 2]]]
    assert blob == [[[2, 1], [2, 2], [4, 2], [4, 4], [2, 4], [2, 2], [1, 2], [1, 1], [2, 1]]]
    assert all(type(c) is int for ring in ground + blob for xy in ring for c in xy), "without a transform the coordinates stay ints"
    # tensors go in as arrays do, and the order of the rings handed in does not matter
    as_tensors = ops.SceneRings(*(torch.from_numpy(np.ascontiguousarray(f)) for f in rings))
    assert gscene.polygons(as_tensors) == features
    shuffled = _as_rings([HAND_RINGS[6][3][k] for k in (3, 2, 1, 0)])
    assert gscene.polygons(shuffled) == features
    assert gscene.polygons(_as_rings([])) == []


def test_polygons_over_the_patterns_have_one_feature_per_component():
    for name in ("rings", "percolation", "ignore-cross"):
        mask, labels, sizes, rings = _case(name, 37, 53, 4, PATTERNS[name][1])
        features = gscene.polygons(rings)
        assert [f["properties"]["label"] for f in features] == np.flatnonzero(sizes).tolist()
        assert [f["properties"]["pixels"] for f in features] == sizes[sizes > 0].tolist()
        assert [f["properties"]["value"] for f in features] == mask.reshape(-1)[np.flatnonzero(sizes)].tolist()
        assert sum(len(f["geometry"]["coordinates"]) for f in features) == len(rings.value)
        assert all(ring[0] == ring[-1] and len(ring) >= 5 for f in features for ring in f["geometry"]["coordinates"])


def test_polygons_transform():
    rings = _as_rings(HAND_RINGS[0][3])      # the single pixel at x = 3, y = 2
    a, b, c, d, e, f = 0.5, 0.0, 100.0, 0.0, -0.5, 2000.0      # a north-up raster of half-metre pixels
    (feature,) = gscene.polygons(rings, (a, b, c, d, e, f))
    assert feature["geometry"]["coordinates"] == [[[102.0, 1999.0], [102.0, 1998.5], [101.5, 1998.5], [101.5, 1999.0], [102.0, 1999.0]]]
    assert feature["properties"] == {"value": 1, "label": 17, "pixels": 1}
    (sheared,) = gscene.polygons(rings, [1, 2, 3, 4, 5, 6])      # (x, y) -> (x + 2 y + 3, 4 x + 5 y + 6)
    assert sheared["geometry"]["coordinates"][0][:2] == [[4 + 2 * 2 + 3, 4 * 4 + 5 * 2 + 6], [4 + 2 * 3 + 3, 4 * 4 + 5 * 3 + 6]]
    for bad in ((1, 2, 3), 5, "abcdef", (1, 2, 3, 4, 5, None)):
        with pytest.raises(ValueError, match="polygons: transform"):
            gscene.polygons(rings, bad)


def test_polygons_refuse_a_broken_ring_set():
    rows = HAND_RINGS[2][3]      # the block with the centre hole
    with pytest.raises(ValueError, match="label 9 has 0 exterior rings"):
        gscene.polygons(_as_rings(rows[1:]))      # the hole alone
    with pytest.raises(ValueError, match="label 9 has 2 exterior rings"):
        gscene.polygons(_as_rings([rows[0], (1, 9, 42, 2, rows[1][4][::-1])]))
    whole = _as_rings(rows)
    with pytest.raises(ValueError, match="do not belong together"):
        gscene.polygons(whole._replace(ring_offsets=whole.ring_offsets[:-1]))
    with pytest.raises(ValueError, match="do not belong together"):
        gscene.polygons(whole._replace(vertices=whole.vertices[:-1]))
