"""GPU tests of the ring simplification of whole-scene inference: ``ops.scene_rings_simplify`` (include/gdlhip_scene_simplify.h),
``SceneInference.predict_rings(simplify=)`` and ``gdlhip.scene.polygons`` on collapsed rings.

Every comparison is exact.  The yardstick is the sequential Douglas-Peucker of tests/_simplify_oracle.py (which
tests/test_scene_simplify_host.py holds against hand-written cases and its own invariants) on the rings of tests/_rings_oracle.py;
the rings and masks are those tests/test_hip_scene_rings.py caches, the dense rings are computed once per mask and shared by the
five tolerances.  Shapes and patterns are those of the rings tests.  The shared-boundary property is asserted as
tests/test_scene_simplify_host.py states it (symmetry at every tolerance, "exactly once" where nothing collapses)."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
import _rings_oracle as ro  # noqa: E402
import _simplify_oracle as sim  # noqa: E402
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402
from gdlhip import scene as gscene  # noqa: E402
from test_hip_scene_rings import CONNECTIVITY, DEV, FIELDS, PATTERNS, SHAPES, _equal, _mask, _rings, _si, dofa, shape_ids  # noqa: E402,F401
from test_scene_simplify_host import RIM, TOLERANCES, shared_boundary  # noqa: E402

ROUNDS = _lib.SCENE_SIMPLIFY_ROUNDS


@functools.lru_cache(maxsize=None)
def _dense(name: str, H: int, W: int, connectivity: int, ignore, values):
    return sim.dense_rings(_rings(name, H, W, connectivity, ignore, values), _mask(name, H, W), -1 if ignore is None else ignore, values)


def _want(name: str, H: int, W: int, connectivity: int, ignore, values, tolerance: float):
    """(the oracle's simplified rings, its depth)."""
    return sim.simplify(_rings(name, H, W, connectivity, ignore, values), _mask(name, H, W), sim.quantise(tolerance),
                        -1 if ignore is None else ignore, values, _dense(name, H, W, connectivity, ignore, values))


def _device(rings: ro.Rings) -> ops.SceneRings:
    return ops.SceneRings(*(torch.from_numpy(f.copy()).to(DEV) for f in rings))


# ------------------------------------------------------------------ 1. the simplified rings of the patterns
@pytest.mark.parametrize("H,W", SHAPES, ids=shape_ids)
@pytest.mark.parametrize("name", list(PATTERNS))
def test_simplified_rings_are_the_oracles(name, H, W):
    host = _mask(name, H, W)
    mask = torch.from_numpy(host.copy()).to(DEV)
    for connectivity in CONNECTIVITY:
        for ignore in (None, PATTERNS[name][1]):
            for values in ((None, (1, 3)) if name == "random-5" else (None,)):
                traced = _rings(name, H, W, connectivity, ignore, values)
                rings = _device(traced)
                for tolerance in TOLERANCES:
                    where = (name, H, W, connectivity, ignore, values, tolerance)
                    got = ops.scene_rings_simplify(rings, mask, tolerance, ignore, values)
                    _equal(got, _want(*where)[0], where)
                    again = ops.scene_rings_simplify(rings, mask, tolerance, ignore, values)      # the same bits from run to run
                    assert all(torch.equal(a, b) for a, b in zip(got, again)), where
                assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(rings, traced)), "the input rings are not modified"
    assert np.array_equal(mask.cpu().numpy(), host), "the mask is not modified"


def test_the_big_cases_are_what_they_are_meant_to_be():
    H, W = SHAPES[0]
    want, depth = _want("spiral", H, W, 4, 0, None, 0.75)      # the arm alone: one free ring of tens of thousands of vertices
    assert len(want.value) == 1 and depth > 2 * ROUNDS, f"depth {depth}: more than two groups of rounds"
    board_mask = torch.from_numpy(_mask("checkerboard", H, W).copy()).to(DEV)
    board = ops.scene_rings(board_mask, 4)
    for tolerance in TOLERANCES:      # H * W rings of four anchors that no tolerance changes
        out = ops.scene_rings_simplify(board, board_mask, tolerance)
        inner = out.ring_offsets.diff() == 4
        assert out.value.numel() == H * W and inner.sum() >= (H - 2) * (W - 2)
        if tolerance == 0:
            assert all(torch.equal(a, b) for a, b in zip(out, board))
    const_mask = torch.full((H, W), 7, dtype=torch.uint8, device=DEV)
    const = ops.scene_rings(const_mask, 8)
    assert ops.scene_rings_simplify(const, const_mask, 1.5).vertices.tolist() == [[W, 0], [W, H], [0, H], [0, 0]]
    alone = ops.scene_rings_simplify(const, const_mask, 300.0)      # above the diagonal (236.6): the ring's one anchor
    assert alone.vertices.tolist() == [[0, 0]] and alone.ring_offsets.tolist() == [0, 1] and alone.area2.tolist() == [2 * H * W]
    assert gscene.polygons(alone) == []


def test_the_wide_comparison_needs_128_bits():
    """A staircase along a 2 x 40 000 mask at tolerance 30 000: tol_q8^2 * |b - a|^2 exceeds 2^64 for the chords tested."""
    W, tolerance = 40000, 30000.0
    host = np.zeros((2, W), dtype=np.uint8)
    host[0, :] = 1
    host[1, 1::2] = 1      # class 1 above, with a tooth into every second pixel of the lower row
    q = sim.quantise(tolerance)
    traced = ro.trace(host)
    dense = sim.dense_rings(traced, host)
    chords = []      # of the arcs that have a candidate: what Douglas-Peucker tests first
    for ring in dense[0]:
        at = sim.anchor_positions(ring, dense[1])
        chords += [(ring[s], ring[e % len(ring)]) for s, e in zip(at, at[1:] + [at[0] + len(ring)]) if e - s > 1]
    assert any(q * q * ((bx - ax) ** 2 + (by - ay) ** 2) > 2 ** 64 for (ax, ay), (bx, by) in chords)
    want, _ = sim.simplify(traced, host, q, dense=dense)
    mask = torch.from_numpy(host).to(DEV)
    got = ops.scene_rings_simplify(ops.scene_rings(mask), mask, tolerance)
    _equal(got, want, "wide")
    fine, _ = sim.simplify(traced, host, sim.quantise(0.25), dense=dense)      # and one tolerance at which the teeth stay
    _equal(ops.scene_rings_simplify(_device(traced), mask, 0.25), fine, "wide, 0.25")
    assert len(fine.vertices) > len(want.vertices)


@pytest.mark.parametrize("name", ["percolation", "random-5"])
def test_neighbours_share_their_simplified_boundary(name):
    H, W = SHAPES[2]
    host = np.pad(_mask(name, H, W), 1, constant_values=RIM)
    mask = torch.from_numpy(host).to(DEV)
    for connectivity in CONNECTIVITY:
        rings = ops.scene_rings(mask, connectivity)
        assert rings.start[0] == 0 and rings.value[0] == RIM, "ring 0 is the frame"
        for tolerance in TOLERANCES:
            out = ops.scene_rings_simplify(rings, mask, tolerance)
            shared_boundary(ro.Rings(*(f.cpu().numpy() for f in out)), tolerance)


def test_no_live_pixel_gives_no_ring():
    mask = torch.full((37, 53), 7, dtype=torch.uint8, device=DEV)
    for kw in (dict(ignore_label=7), dict(values=[])):
        got = ops.scene_rings_simplify(ops.scene_rings(mask, **kw), mask, 1.5, **kw)
        assert tuple(got.vertices.shape) == (0, 2) and got.ring_offsets.tolist() == [0], kw
        assert all(getattr(got, f).numel() == 0 and getattr(got, f).dtype == FIELDS[f] and getattr(got, f).is_cuda for f in FIELDS if
                   f != "ring_offsets"), kw
        assert gscene.polygons(got) == []


SCAN_TILE = _lib.SCENE_SIMPLIFY_SCAN_TILE


def _islands(pixels: int, trominoes: int, teeth: int) -> np.ndarray:
    """Islands on a pitch of three pixels in a sea of 0 (ignored by the caller), so that V and D are known by counting: a single
    pixel is a ring of 4 vertices, an L of three pixels one of 6, and a `tooth` -- a domino of class 1 on a pixel of class 2 under
    its left half -- two rings of 4 with one node strictly inside the domino's lower run: 8 vertices, 9 dense ones."""
    n = pixels + trominoes + teeth
    side = int(np.ceil(np.sqrt(n)))
    m = np.zeros((3 * side, 3 * side), dtype=np.uint8)
    for i in range(n):
        y, x = 3 * (i // side), 3 * (i % side)
        m[y, x] = 1
        if i >= pixels:
            m[y, x + 1] = 1
            m[y + 1, x] = 1 if i < pixels + trominoes else 2
    return m


# V is even (the rings are rectilinear), so V + 1 is SCAN_TILE - 1 or SCAN_TILE + 1; D + 1 takes all three values around it
@pytest.mark.parametrize("pixels,trominoes,teeth,V,D", [(510, 1, 0, SCAN_TILE - 2, SCAN_TILE - 2), (508, 1, 1, SCAN_TILE - 2, SCAN_TILE - 1),
                                                        (506, 1, 2, SCAN_TILE - 2, SCAN_TILE), (512, 0, 0, SCAN_TILE, SCAN_TILE)])
def test_the_scans_at_their_block_boundaries(pixels, trominoes, teeth, V, D):
    """gdl_scene_simplify_count scans V + 1 entries, _dense and _write D + 1, in blocks of SCAN_TILE: the last block full but
    for one entry, exactly full, and a second block of one entry, which holds the total the next call is sized by."""
    host = _islands(pixels, trominoes, teeth)
    assert host.size < 5000
    traced = ro.trace(host, 4, 0)
    dense = sim.dense_rings(traced, host, 0)
    assert (len(traced.vertices), sum(len(ring) for ring in dense[0])) == (V, D)
    mask = torch.from_numpy(host).to(DEV)
    rings = ops.scene_rings(mask, 4, 0)
    _equal(rings, traced, "islands")
    for tolerance in (0, 0.75):      # what lies on its chord alone, and a tolerance that takes corners of the islands
        where = (pixels, trominoes, teeth, tolerance)
        _equal(ops.scene_rings_simplify(rings, mask, tolerance, 0), sim.simplify(traced, host, sim.quantise(tolerance), 0, dense=dense)[0], where)


# ------------------------------------------------------------------ 2. SceneInference, DOFA, end to end
def test_predict_rings_simplify(dofa):  # noqa: F811
    nc, img, sm, scene = dofa
    si = _si(dofa)
    plain = si.predict_rings(scene)
    none = si.predict_rings(scene, simplify=None)
    assert torch.equal(none.mask, plain.mask) and all(torch.equal(a, b) for a, b in zip(none.rings, plain.rings))
    res = si.predict_rings(scene, simplify=1.5)
    by_hand = ops.scene_rings_simplify(plain.rings, plain.mask, 1.5)
    assert torch.equal(res.mask, plain.mask) and all(torch.equal(a, b) for a, b in zip(res.rings, by_hand))
    host = plain.mask.cpu().numpy()
    _equal(res.rings, sim.simplify(ro.trace(host), host, sim.quantise(1.5))[0], "end to end")
    assert res.rings.vertices.shape[0] < plain.rings.vertices.shape[0]
    before, after = gscene.polygons(plain.rings), gscene.polygons(res.rings)
    pixels = {f["properties"]["label"]: f["properties"]["pixels"] for f in before}
    counts = (res.rings.ring_offsets.diff()).tolist()
    remaining = sorted(lab for lab, n, a in zip(res.rings.label.tolist(), counts, res.rings.area2.tolist()) if a > 0 and n >= 3)
    assert [f["properties"]["label"] for f in after] == remaining, "one exterior per remaining label"
    for f in after:
        assert f["properties"]["pixels"] == pixels[f["properties"]["label"]], "pixels are those of the unsimplified feature"
        assert all(ring[0] == ring[-1] and len(ring) >= 4 for ring in f["geometry"]["coordinates"]), "closed rings"
