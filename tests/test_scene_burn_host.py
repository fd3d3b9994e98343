"""Host side of burning polygon rings into a label raster, no GPU: the binding of include/gdlhip_scene_burn.h
(SCENE_BURN_SIGNATURES) beside the other sets, the refusals that fire before anything touches a device, the integer restatement
the GPU tests compare with (tests/_burn_oracle.py) held against results written out by hand and against the round trip through
the ring tracer of tests/_rings_oracle.py, and ``gdlhip.scene.rings_from_features``, the inverse of ``polygons``."""

import ctypes as C

import numpy as np
import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
import _burn_oracle as bo  # noqa: E402
import _rings_oracle as ro  # noqa: E402
import _sieve_oracle as so  # noqa: E402
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402
from gdlhip import scene as gscene  # noqa: E402
from geo_deep_learning.tools import scene_inference as si  # noqa: E402

NAMES = ["gdl_scene_burn_count", "gdl_scene_burn_fill"]


# ------------------------------------------------------------------ the binding and the checks without a device
def test_burn_header_is_bound_beside_the_other_sets():
    i, l, p = C.c_int, C.c_int64, C.c_void_p
    sig = _lib.SCENE_BURN_SIGNATURES
    assert sorted(sig) == NAMES
    assert sig["gdl_scene_burn_count"] == (i, [p, p, i, i, i, i, i, p, p, p, p, p])
    assert sig["gdl_scene_burn_fill"] == (i, [p, p, p, i, i, i, i, i, p, p, l, i, i, p, p, p, p, p])
    for other in (_lib.SIGNATURES, _lib.DEBUG_SIGNATURES, _lib.SCENE_SIGNATURES, _lib.SCENE_TTA_SIGNATURES, _lib.SCENE_NODATA_SIGNATURES,
                  _lib.SCENE_SIEVE_SIGNATURES, _lib.SCENE_RINGS_SIGNATURES, _lib.SCENE_SIMPLIFY_SIGNATURES, _lib.SCENE_REGIONS_SIGNATURES):
        assert not set(sig) & set(other)
    assert not set(sig) & _lib.STATUS_FUNCTIONS and set(sig) <= _lib._CHECKED
    assert _lib.SCENE_BURN_SCAN_TILE == _lib.SCENE_RINGS_SCAN_TILE == 2048 and _lib.SCENE_BURN_BITS_MAX == 8 and _lib.SCENE_BURN_CHUNK == 256
    assert len(_lib.SCENE_REGIONS_SIGNATURES) == 2 and len(_lib.SCENE_RINGS_SIGNATURES) == 3      # the siblings keep their sizes


def test_burn_functions_are_exported_and_refuse_before_any_launch():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    raw, checked = _lib.load(), _lib.checked()
    for n, (res, args) in _lib.SCENE_BURN_SIGNATURES.items():
        assert getattr(raw, n).argtypes == args and getattr(raw, n).restype is res
        assert getattr(checked, n).errcheck is _lib.status_errcheck
    buf = (C.c_char * 64)()
    a = C.addressof(buf)      # never followed: every call below is refused first

    def count(H=4, W=4, R=1, V=4, bits=0, ptr=(a,) * 6):
        v, off, ring, rows, bsum, counts = ptr
        return raw.gdl_scene_burn_count(v, off, R, V, bits, H, W, ring, rows, bsum, counts, None)

    def fill(H=4, W=4, R=1, V=4, bits=0, n_cross=4, background=0, conflict=255, ptr=(a,) * 9):
        v, off, val, ring, rows, ref, plane, out, counts = ptr
        return raw.gdl_scene_burn_fill(v, off, val, R, V, bits, H, W, ring, rows, n_cross, background, conflict, ref, plane, out, counts, None)

    for name, call in (("gdl_scene_burn_count", count), ("gdl_scene_burn_fill", fill)):
        for H, W in ((65536, 32768), (2, 2 ** 30), (46341, 46341)):      # H * W >= 2^31
            assert call(H=H, W=W) == -1
            assert f"{name}: {H} x {W} pixels".encode() in raw.gdl_last_error() and b"2^31" in raw.gdl_last_error()
        for H, W in ((0, 4), (4, 0), (-1, 4)):
            assert call(H=H, W=W) == -1 and f"{name}: bad sizes".encode() in raw.gdl_last_error()
        for bits in (-1, 9):
            assert call(bits=bits) == -1 and f"{name}: bits must be in 0..8, got {bits}".encode() in raw.gdl_last_error()
        for R, V in ((-1, 4), (1, -1)):
            assert call(R=R, V=V) == -1 and f"{name}: {R} rings and {V} vertices".encode() in raw.gdl_last_error()
    for k in range(6):      # every pointer of the count is needed while there are vertices
        assert count(ptr=tuple(None if j == k else a for j in range(6))) == -1 and b"gdl_scene_burn_count: null pointer" in raw.gdl_last_error()
    for k in (0, 1, 2, 3, 4, 6, 7, 8):      # and every one of the fill but the reference
        assert fill(ptr=tuple(None if j == k else a for j in range(9))) == -1 and b"gdl_scene_burn_fill: null pointer" in raw.gdl_last_error()
    for k in (7, 8):      # out and counts also where nothing is to burn
        assert fill(n_cross=0, ptr=tuple(None if j == k else a for j in range(9))) == -1 and b"null pointer" in raw.gdl_last_error()
    for background, conflict in ((-1, 255), (256, 255), (0, -1), (0, 256)):
        assert fill(background=background, conflict=conflict) == -1
        assert f"gdl_scene_burn_fill: background and conflict must be in 0..255, got {background} and {conflict}".encode() in raw.gdl_last_error()
    for n in (-1, 2 ** 31, 2 ** 40):
        assert fill(n_cross=n) == -1 and f"gdl_scene_burn_fill: {n} crossings".encode() in raw.gdl_last_error()
    assert fill(ptr=(a,) * 6 + (a + 4, a, a)) == -1 and b"plane must be 16-byte aligned" in raw.gdl_last_error()
    with pytest.raises(ValueError, match="gdl_scene_burn_fill: bits must be in 0..8, got 9"):
        checked.gdl_scene_burn_fill(a, a, a, 1, 4, 9, 4, 4, a, a, 4, 0, 255, a, a, a, a, None)


def test_ops_scene_burn_checks_its_arguments_before_a_device_is_needed():
    rings = bo.make([(3, [(0, 0), (2, 0), (2, 2)])])
    t = gscene.FeatureRings(*(torch.from_numpy(f) for f in rings))
    op = "scene_burn"
    with pytest.raises(ValueError, match="device tensors"):      # every argument is fine: the device is asked for last
        ops.scene_burn(t, (4, 5), bits=8, background=7, conflict=9, reference=torch.zeros((4, 5), dtype=torch.uint8))
    with pytest.raises(ValueError, match=f"{op}: rings must have the tensor fields vertices, ring_offsets, value"):
        ops.scene_burn(rings, (4, 5))      # numpy arrays
    for bad in (t._replace(vertices=t.vertices.long()), t._replace(vertices=t.vertices.reshape(-1)), t._replace(value=t.value.int()),
                t._replace(value=torch.zeros(2, dtype=torch.uint8)), t._replace(ring_offsets=t.ring_offsets.long()),
                t._replace(vertices=t.vertices.t().contiguous().t())):
        with pytest.raises(ValueError, match=f"{op}: rings\\.\\w+ must be a contiguous"):
            ops.scene_burn(bad, (4, 5))
    for bad in ((0, 5), (4, 0), (4,), 4, (4.0, 5), (True, 5), None):
        with pytest.raises(ValueError, match=f"{op}: size must be \\(H, W\\)"):
            ops.scene_burn(t, bad)
    with pytest.raises(ValueError, match=f"{op}: 65536 x 32768 pixels"):
        ops.scene_burn(t, (65536, 32768))
    for bad in (-1, 9, 1.0, True):
        with pytest.raises(ValueError, match=f"{op}: bits must be an int in 0..8"):
            ops.scene_burn(t, (4, 5), bits=bad)
    for kw in (dict(background=256), dict(background=-1), dict(conflict=256), dict(conflict=1.5), dict(conflict=True)):
        with pytest.raises(ValueError, match=f"{op}: {list(kw)[0]} must be an int in 0..255"):
            ops.scene_burn(t, (4, 5), **kw)
    for bad in (torch.zeros((4, 5)), torch.zeros((5, 4), dtype=torch.uint8), torch.zeros((5, 4), dtype=torch.uint8).t(), np.zeros((4, 5), np.uint8)):
        with pytest.raises(ValueError, match=f"{op}: reference must be a contiguous uint8 / bool \\[H, W\\] = \\[4, 5\\]"):
            ops.scene_burn(t, (4, 5), reference=bad)
    assert ops.SceneBurn._fields == ("mask", "conflicts", "differ") == bo.Burn._fields
    # a two-vertex ring passes where _rings_check would not
    small = gscene.FeatureRings(*(torch.from_numpy(f) for f in bo.make([(3, [(0, 0), (2, 0)])])))
    with pytest.raises(ValueError, match="device tensors"):
        ops.scene_burn(small, (4, 5))
    assert si.SceneVectorsAgreement._fields == ("mask", "rings", "agreement") and si.SceneVectors._fields == ("mask", "rings")
    assert si.SceneFeaturesAgreement._fields == ("mask", "rings", "regions", "agreement") and si.SceneFeatures._fields == ("mask", "rings", "regions")
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="rings_agreement: num_classes must be an int in 1..64"):
            si.rings_agreement(torch.zeros((4, 5), dtype=torch.uint8), t, bad)
    with pytest.raises(ValueError, match="device tensors"):
        si.rings_agreement(torch.zeros((4, 5), dtype=torch.uint8), t, 5)


# ------------------------------------------------------------------ the oracle, by hand
@pytest.mark.parametrize("name,rings,bits,kw,want,conflicts", bo.HAND_CASES, ids=[c[0] for c in bo.HAND_CASES])
def test_the_oracle_on_hand_drawn_cases(name, rings, bits, kw, want, conflicts):
    H, W = want.shape
    for shift in (0, 1, 8 - bits):
        got = bo.burn(bo.make(rings, 1 << shift), H, W, bits + shift, **kw)
        assert np.array_equal(got.mask, want) and got.mask.dtype == np.uint8, f"\n{got.mask}\n{want}"
        assert got.conflicts == conflicts == int((want == 9).sum()) and got.differ is None
        assert bo.burn(bo.make(rings[::-1], 1 << shift), H, W, bits + shift, reference=want, **kw).differ == 0      # order-free


def test_the_hand_cases_cover_what_they_are_for():
    names = " / ".join(c[0] for c in bo.HAND_CASES)
    for what in ("unit square", "hole", "island", "triangles", "overlapping", "reversed", "two vertices", "clipped", "centre lines"):
        assert what in names, what
    clipped = [c for c in bo.HAND_CASES if c[0] == "clipped on all four sides"][0]
    found = bo.crossings(bo.make(clipped[1]), 3, 4)
    assert sorted(found) == [(y, 0, 1, 2) for y in range(3)]      # x0 = -2 clamped to 0, x0 = 6 dropped
    rim = [c for c in bo.HAND_CASES if c[0] == "beyond the right and lower rim"][0]
    assert sorted(bo.crossings(bo.make(rim[1]), 3, 3)) == [(1, 2, 1, 1), (2, 2, 1, 1)]
    tri = bo.make([c for c in bo.HAND_CASES if "triangles" in c[0]][0][1])
    assert len(bo.crossings(tri, 4, 4)) == 4 * 4 - 4      # the right edge at x = 4 is dropped
    assert bo.bad_entries(tri) == 0 and bo.bad_entries(tri._replace(ring_offsets=np.array([0, 4, 3]))) == 1
    assert bo.bad_entries(tri._replace(ring_offsets=np.array([-1, 3, 7]))) == 2
    far = tri._replace(vertices=tri.vertices * 2 ** 20)
    assert bo.bad_entries(far) == 6 and bo.bad_entries(far, bits=2) == 0      # the six coordinates that are not 0
    assert bo.bad_entries(tri._replace(vertices=tri.vertices * 2 ** 18)) == 0      # 2^20 itself is in range


# ------------------------------------------------------------------ the oracle, round trips
@pytest.mark.parametrize("name", list(so.patterns(16)))
def test_burning_the_traced_rings_gives_the_mask_back(name):
    make, ignore = so.patterns(16)[name]
    for H, W in ((23, 31), (1, 9), (9, 1)):
        mask = make(H, W)
        for connectivity in (4, 8):
            rings = ro.trace(mask, connectivity)
            got = bo.burn(rings, H, W, background=200, conflict=201, reference=mask)
            assert np.array_equal(got.mask, mask) and got.conflicts == 0 and got.differ == 0, (name, H, W, connectivity)
            assert np.array_equal(np.where(ro.fill(rings, H, W) >= 0, mask, 200), got.mask)      # the unit-step fill agrees
            # ignored pixels have no ring and become background
            part = bo.burn(ro.trace(mask, connectivity, ignore_label=ignore), H, W, background=ignore)
            assert np.array_equal(part.mask, mask) and part.conflicts == 0
            # values=: the classes left out become background, holes whose islands are missing included
            keep = [int(v) for v in np.unique(mask)[:1]]
            some = bo.burn(ro.trace(mask, connectivity, values=keep), H, W, background=7)
            assert np.array_equal(some.mask, np.where(np.isin(mask, keep), mask, 7)) and some.conflicts == 0


@pytest.mark.parametrize("shift", [1, 8])
def test_scaled_rings_with_bits_give_the_same_raster(shift):
    for name in ("random-5", "rings", "percolation"):
        mask = so.patterns(16)[name][0](19, 27)
        rings = ro.trace(mask, 8)
        scaled = bo.Rings(rings.vertices * (1 << shift), rings.ring_offsets, rings.value)
        assert np.array_equal(bo.burn(scaled, 19, 27, bits=shift, background=9).mask, mask)


@pytest.mark.parametrize("seed", range(6))
def test_a_fan_of_triangles_partitions_the_rectangle(seed):
    for H, W in ((7, 11), (1, 5), (16, 3)):
        got = bo.burn(bo.fan(H, W, seed), H, W, bits=8, background=0, conflict=255)
        assert got.conflicts == 0 and got.mask.min() >= 1 and got.mask.max() <= 5, f"\n{got.mask}"


# ------------------------------------------------------------------ rings_from_features
def _ring_set(rings) -> list:
    v, off, val = (np.asarray(f).tolist() for f in (rings.vertices, rings.ring_offsets, rings.value))
    out = []
    for r in range(len(val)):
        ring = [tuple(p) for p in v[off[r]:off[r + 1]]]
        k = ring.index(min(ring))
        out.append((val[r], tuple(ring[k:] + ring[:k])))      # up to rotation
    return sorted(out)


@pytest.mark.parametrize("name", ["random-5", "rings", "ignore-cross", "spiral"])
def test_rings_from_features_inverts_polygons(name):
    make, ignore = so.patterns(16)[name]
    mask = make(21, 17)
    rings = ro.trace(mask, 4, ignore_label=ignore)
    back = gscene.rings_from_features(gscene.polygons(rings))
    assert isinstance(back, gscene.FeatureRings) and [t.dtype for t in back] == [torch.int32, torch.int32, torch.uint8]
    assert back.vertices.shape == rings.vertices.shape and back.ring_offsets.shape == rings.ring_offsets.shape
    assert _ring_set(back) == _ring_set(rings)
    host = bo.Rings(*(t.numpy() for t in back))
    assert np.array_equal(bo.burn(host, 21, 17, background=ignore).mask, mask)
    # through a transform and back: a north-up grid of 0.5 m pixels, and one with rotation terms
    for t in ((0.5, 0.0, 500000.0, 0.0, -0.5, 4000000.0), (3.0, 1.0, -7.0, -1.0, 2.0, 11.0)):
        moved = gscene.rings_from_features(gscene.polygons(rings, transform=t), transform=t)
        assert _ring_set(moved) == _ring_set(rings)
        fine = gscene.rings_from_features({"type": "FeatureCollection", "features": gscene.polygons(rings, transform=t)}, transform=t, bits=3)
        assert torch.equal(fine.vertices, moved.vertices * 8) and torch.equal(fine.ring_offsets, moved.ring_offsets)


def test_rings_from_features_orients_strips_and_rounds():
    square = [[1, 1], [1, 3], [3, 3], [3, 1], [1, 1]]      # closed, and the wrong way round for an exterior
    hole = [[1.5, 1.5], [2.5, 1.5], [2.5, 2.5], [1.5, 2.5]]      # open, and the wrong way round for a hole
    feats = [{"type": "Feature", "properties": {"value": 4, "class": 9}, "geometry": {"type": "Polygon", "coordinates": [square, hole]}},
             {"type": "Feature", "properties": {"value": 6, "class": 2},
              "geometry": {"type": "MultiPolygon", "coordinates": [[[[0, 0], [1, 0], [1, 1]]], [[[3, 3, 50.0], [4, 3, 50.0], [4, 4, 50.0]]]]}}]
    got = gscene.rings_from_features(feats, bits=1)
    assert got.ring_offsets.tolist() == [0, 4, 8, 11, 14] and got.value.tolist() == [4, 4, 6, 6]
    v = [tuple(q) for q in got.vertices.tolist()]
    assert v[:4] == [(6, 2), (6, 6), (2, 6), (2, 2)] and v[4:8] == [(3, 5), (5, 5), (5, 3), (3, 3)]      # both reversed
    assert v[8:] == [(0, 0), (2, 0), (2, 2), (6, 6), (8, 6), (8, 8)]      # as given: the third coordinate is dropped
    area2 = lambda ring: sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(ring, ring[1:] + ring[:1]))      # noqa: E731
    assert area2(v[:4]) > 0 > area2(v[4:8]) and area2(v[8:11]) > 0
    # the hole 1.5 .. 2.5 has its corners on the centres of four pixels: (1, 1) lies right of its left edge, inside the hole; the
    # others lie on its right edge or below its rows.  Each hypotenuse passes through one centre, right of it: in the triangle
    burned = bo.burn(bo.Rings(*(t.numpy() for t in got)), 4, 4, bits=1)
    assert burned.mask.tolist() == [[6, 0, 0, 0], [0, 0, 4, 0], [0, 4, 4, 0], [0, 0, 0, 6]] and burned.conflicts == 0
    assert gscene.rings_from_features(feats, value_key="class").value.tolist() == [9, 9, 2, 2]
    assert gscene.rings_from_features(feats, bits=0).vertices.tolist()[4:8] == [[2, 3], [3, 3], [3, 2], [2, 2]]      # halves go up
    empty = gscene.rings_from_features([])
    assert empty.vertices.shape == (0, 2) and empty.ring_offsets.tolist() == [0] and empty.value.shape == (0,)


def test_rings_from_features_refuses_what_it_cannot_read():
    ring = [[0, 0], [1, 0], [1, 1]]
    ok = {"type": "Feature", "properties": {"value": 1}, "geometry": {"type": "Polygon", "coordinates": [ring]}}
    assert gscene.rings_from_features([ok]).value.tolist() == [1]
    with pytest.raises(ValueError, match="rings_from_features: feature 1 has no property 'value'"):
        gscene.rings_from_features([ok, {**ok, "properties": {"label": 3}}])
    with pytest.raises(ValueError, match="rings_from_features: feature 0 has no property 'klass'"):
        gscene.rings_from_features([ok], value_key="klass")
    for bad in (-1, 256, 1.0, "1", True, None):
        with pytest.raises(ValueError, match="rings_from_features: feature 0: value must be an int in 0..255"):
            gscene.rings_from_features([{**ok, "properties": {"value": bad}}])
    for t in ((1.0, 2.0, 0.0, 2.0, 4.0, 0.0), (0.0, 0.0, 1.0, 0.0, 0.0, 1.0), (1.0, 0.0, float("nan"), 0.0, 1.0, 0.0)):
        with pytest.raises(ValueError, match="rings_from_features: the transform .* is singular"):
            gscene.rings_from_features([ok], transform=t)
    with pytest.raises(ValueError, match="rings_from_features: transform must be None or six numbers"):
        gscene.rings_from_features([ok], transform=(1.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="rings_from_features: feature 0: a Polygon or MultiPolygon geometry is expected, got 'Point'"):
        gscene.rings_from_features([{**ok, "geometry": {"type": "Point", "coordinates": [0, 0]}}])
    for bad in (-1, 9, 1.0):
        with pytest.raises(ValueError, match="rings_from_features: bits must be an int in 0..8"):
            gscene.rings_from_features([ok], bits=bad)
