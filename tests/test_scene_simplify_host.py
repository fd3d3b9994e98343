"""Host side of the ring simplification of whole-scene inference, no GPU: the binding of include/gdlhip_scene_simplify.h
(SCENE_SIMPLIFY_SIGNATURES), the argument checks that fire before anything touches a device, the new rule of
``gdlhip.scene.polygons`` for collapsed rings, and the sequential oracle the GPU tests compare with (tests/_simplify_oracle.py)
held against cases written out by hand and against its own invariants.

The shared-boundary property is stated as it holds.  Every arc is traced by the two rings on its sides, once in each direction,
and simplified to the same points: the multiset of the directed segments of all rings but the frame is therefore symmetric under
reversal, at every tolerance, and that is asserted.  "Every segment occurs exactly once" holds only while no two arcs have been
simplified onto one chord: two arcs between the same two nodes (a region one pixel wide) or the two halves of a closed arc (an
island that collapses to two vertices) give the same segment twice in each direction.  On the 37 x 53 patterns that happens from
tolerance 0.75 on (percolation: 142 of 1826 segments, diagonal-lines: 898 of 1238), so "exactly once" is asserted at tolerance
0, where nothing collapses, and the symmetry at all five: ``test_neighbours_share_their_simplified_boundary``."""

import ctypes as C
import functools
from collections import Counter

import numpy as np
import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
import _rings_oracle as ro  # noqa: E402
import _sieve_oracle as so  # noqa: E402
import _simplify_oracle as sim  # noqa: E402
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402
from gdlhip import scene as gscene  # noqa: E402
from geo_deep_learning.tools.scene_inference import SceneInference  # noqa: E402

NAMES = ["gdl_scene_nodes", "gdl_scene_simplify_count", "gdl_scene_simplify_dense", "gdl_scene_simplify_rounds", "gdl_scene_simplify_write"]
PATTERNS = so.patterns(64)
SHAPE = (37, 53)
TOLERANCES = [0, 0.75, 1.5, 4, 1000]
RIM = 200      # a class no pattern uses


# ------------------------------------------------------------------ the binding and the checks without a device
def test_simplify_header_is_bound_beside_the_other_sets():
    i, p = C.c_int, C.c_void_p
    sig = _lib.SCENE_SIMPLIFY_SIGNATURES
    assert sorted(sig) == NAMES
    assert sig["gdl_scene_nodes"] == (i, [p, i, i, i, p, p, p])
    assert sig["gdl_scene_simplify_count"] == (i, [p, i, i, p, p, i, i, p, p, p, p])
    assert sig["gdl_scene_simplify_dense"] == (i, [p, i, i, p, p, i, i, p, i, p, p, p, p, p, p, p])
    assert sig["gdl_scene_simplify_rounds"] == (i, [p, i, i, i, i, i, p, p, p, p, p])
    assert sig["gdl_scene_simplify_write"] == (i, [p, p, i, i, p, p, p, p, p, p])
    for other in (_lib.SIGNATURES, _lib.DEBUG_SIGNATURES, _lib.SCENE_SIGNATURES, _lib.SCENE_TTA_SIGNATURES, _lib.SCENE_NODATA_SIGNATURES,
                  _lib.SCENE_SIEVE_SIGNATURES, _lib.SCENE_RINGS_SIGNATURES):
        assert not set(sig) & set(other)
    assert not set(sig) & _lib.STATUS_FUNCTIONS and set(sig) <= _lib._CHECKED
    assert (_lib.SCENE_SIMPLIFY_SCAN_TILE, _lib.SCENE_SIMPLIFY_ROUNDS) == (2048, 8)
    assert len(_lib.SCENE_RINGS_SIGNATURES) == 3      # the rings' set keeps its size


def test_simplify_functions_are_exported_and_refuse_before_any_launch():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    raw, checked = _lib.load(), _lib.checked()
    for n, (res, args) in _lib.SCENE_SIMPLIFY_SIGNATURES.items():
        assert getattr(raw, n).argtypes == args and getattr(raw, n).restype is res
        assert getattr(checked, n).errcheck is _lib.status_errcheck
    buf = (C.c_char * 64)()
    a = C.addressof(buf)      # never followed: every call below is refused first
    assert raw.gdl_scene_nodes(a, 4, 4, -1, a, None, None) == -1 and b"gdl_scene_nodes: null pointer" in raw.gdl_last_error()
    assert raw.gdl_scene_nodes(a, 4, 4, 256, a, a, None) == -1 and b"ignore_label 256" in raw.gdl_last_error()
    count = lambda H, W, R, V: raw.gdl_scene_simplify_count(a, H, W, a, a, R, V, a, a, a, None)      # noqa: E731
    dense = lambda H, W, R, V, D: raw.gdl_scene_simplify_dense(a, H, W, a, a, R, V, a, D, a, a, a, a, a, a, None)      # noqa: E731
    rounds = lambda W, D, tol, n: raw.gdl_scene_simplify_rounds(a, W, D, tol, 1, n, a, a, a, a, None)      # noqa: E731
    for H, W in ((32768, 16384), (2, 2 ** 28)):      # H * W >= 2^29
        assert raw.gdl_scene_nodes(a, H, W, -1, a, a, None) == -1 and b"2^29" in raw.gdl_last_error()
        assert count(H, W, 1, 4) == -1 and b"2^29" in raw.gdl_last_error()
    for H, W in ((0, 4), (4, 0), (-1, 4)):
        assert count(H, W, 1, 4) == -1 and b"gdl_scene_simplify_count: bad sizes" in raw.gdl_last_error()
    for R, V in ((1, 3), (0, 4), (1, 0), (-1, 4), (2, 7), (1, 65)):      # counts no mask of 4 x 4 can give
        assert count(4, 4, R, V) == -1 and b"do not belong together" in raw.gdl_last_error(), (R, V)
        assert dense(4, 4, R, V, 8) == -1, (R, V)
    assert dense(4, 4, 1, 8, 7) == -1 and b"gdl_scene_simplify_dense: 7 dense vertices of 8" in raw.gdl_last_error()
    assert dense(4, 4, 0, 0, 0) == -1 and b"no rings" in raw.gdl_last_error()
    assert raw.gdl_scene_simplify_count(a, 4, 4, a, a, 1, 4, None, a, a, None) == -1 and b"null pointer" in raw.gdl_last_error()
    for tol in (-1, 2 ** 28 + 1):
        assert rounds(4, 4, tol, 8) == -1 and f"tol_q8 {tol}".encode() in raw.gdl_last_error()
    for n in (0, 9):
        assert rounds(4, 4, 256, n) == -1 and f"n_rounds {n} is not in 1..8".encode() in raw.gdl_last_error()
    assert rounds(4, 0, 256, 8) == -1 and raw.gdl_scene_simplify_rounds(a, 4, 4, 256, 1, 8, a, a, a, None, None) == -1
    assert raw.gdl_scene_simplify_write(a, a, 2, 7, a, a, a, a, a, None) == -1 and b"do not belong together" in raw.gdl_last_error()
    assert raw.gdl_scene_simplify_write(a, a, 1, 4, a, None, a, a, a, None) == -1 and b"null pointer" in raw.gdl_last_error()
    with pytest.raises(ValueError, match="gdl_scene_simplify_rounds: n_rounds 9"):
        checked.gdl_scene_simplify_rounds(a, 4, 4, 256, 1, 9, a, a, a, a, None)


def _host_rings(mask: np.ndarray, **kw) -> ops.SceneRings:
    return ops.SceneRings(*(torch.from_numpy(f.copy()) for f in ro.trace(mask, **kw)))


def test_ops_and_predict_rings_check_their_arguments_before_the_device():
    host = PATTERNS["random-5"][0](5, 7)
    mask, rings = torch.from_numpy(host), _host_rings(host)
    with pytest.raises(ValueError, match="device tensors"):      # every argument is fine: the device is asked for last
        ops.scene_rings_simplify(rings, mask, 1.5, 3, values=range(5))
    for tol in (-0.5, float("nan"), float("inf"), 2 ** 20 + 1, "1", None, True, [1.0]):
        with pytest.raises(ValueError, match="scene_rings_simplify: tolerance"):
            ops.scene_rings_simplify(rings, mask, tol)
    broken = [rings._replace(vertices=rings.vertices.long()), rings._replace(vertices=rings.vertices.reshape(-1)),
              rings._replace(vertices=rings.vertices[:-1]) if len(rings.value) == 1 else rings._replace(ring_offsets=rings.ring_offsets[:-1]),
              rings._replace(value=rings.value.int()), rings._replace(label=rings.label[:-1]), rings._replace(start=rings.start.long()),
              rings._replace(area2=rings.area2.int()), rings._replace(vertices=rings.vertices.t().contiguous().t()),
              rings._replace(area2=rings.area2.numpy()), rings._replace(vertices=rings.vertices[:3], ring_offsets=rings.ring_offsets[:2],
                                                                        value=rings.value[:1], label=rings.label[:1],
                                                                        start=rings.start[:1], area2=rings.area2[:1]),
              tuple(rings), None]
    for bad in broken:
        with pytest.raises(ValueError, match="scene_rings_simplify: "):
            ops.scene_rings_simplify(bad, mask, 1.5)
    if torch.cuda.is_available():      # fields on two devices
        with pytest.raises(ValueError, match="scene_rings_simplify: rings.ring_offsets"):
            ops.scene_rings_simplify(rings._replace(vertices=rings.vertices.cuda()), mask, 1.5)
    for other in (mask.float(), mask[None], mask.t(), host, torch.zeros((0, 7), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="scene_rings_simplify: .*mask"):
            ops.scene_rings_simplify(rings, other, 1.5)
    with pytest.raises(ValueError, match="scene_rings_simplify: .*pixel sides"):      # more vertices than the mask has sides
        ops.scene_rings_simplify(rings, mask[:1, :1].contiguous(), 1.5)
    with pytest.raises(ValueError, match="2\\^29"):
        ops.scene_rings_simplify(rings, torch.empty((2, 2 ** 28), dtype=torch.uint8, device="meta"), 1.5)
    for kw in (dict(ignore_label=256), dict(ignore_label=True), dict(values=[256]), dict(values=3)):
        with pytest.raises(ValueError):
            ops.scene_rings_simplify(rings, mask, 1.5, **kw)
    assert ops.SIMPLIFY_TOLERANCE_MAX == sim.TOL_MAX == 2 ** 20

    class Stub:      # predict_rings refuses the tolerance before it looks at the raster or the model
        nodata = None
    for tol in (-1, float("nan"), float("inf"), 2 ** 21, "2", True):
        with pytest.raises(ValueError, match="predict_rings: simplify"):
            SceneInference.predict_rings(Stub(), None, simplify=tol)


def test_polygons_leave_collapsed_rings_out():
    # label 0: an exterior with two holes, one of them collapsed to two vertices; label 9: an island collapsed to one vertex
    rings = ro.Rings(np.array([(8, 0), (8, 8), (0, 8), (0, 0), (2, 2), (2, 4), (4, 4), (4, 2), (5, 5), (6, 6), (5, 5)], dtype=np.int32),
                     np.array([0, 4, 8, 10, 11], dtype=np.int32), np.array([1, 1, 1, 2], dtype=np.uint8),
                     np.array([0, 0, 0, 9], dtype=np.int32), np.array([0, 40, 90, 36], dtype=np.int32),
                     np.array([128, -8, -2, 2], dtype=np.int64))
    (feature,) = gscene.polygons(rings)
    assert feature["properties"] == {"value": 1, "label": 0, "pixels": 59}, "pixels stay those of the pixel rings"
    assert feature["geometry"]["coordinates"] == [[[8, 0], [8, 8], [0, 8], [0, 0], [8, 0]], [[2, 2], [2, 4], [4, 4], [4, 2], [2, 2]]]
    gone = rings._replace(ring_offsets=np.array([0, 2, 6, 8, 11], dtype=np.int32))      # the exterior of label 0 collapsed
    (island,) = gscene.polygons(gone)
    assert island["properties"]["label"] == 9 and len(island["geometry"]["coordinates"]) == 1
    with pytest.raises(ValueError, match="exterior rings"):      # still refused: no exterior at all
        gscene.polygons(rings._replace(area2=np.array([-128, -8, -2, 2], dtype=np.int64)))


# ------------------------------------------------------------------ the oracle on hand-written cases
def _rows(*rows: str) -> np.ndarray:
    return np.array([[int(c) for c in r] for r in rows], dtype=np.uint8)


def _simplified(mask: np.ndarray, tolerance: float, **kw) -> list:
    ignore, values = kw.get("ignore_label", -1), kw.get("values")
    out, _ = sim.simplify(ro.trace(mask, kw.get("connectivity", 4), ignore, values), mask, sim.quantise(tolerance), ignore, values)
    return sim.ring_list(out)


def test_a_t_junction_is_inserted_into_the_straight_ring():
    mask = _rows("11", "23")
    node = sim.nodes(mask)
    assert sorted(zip(*np.nonzero(node)[::-1])) == [(0, 1), (1, 1), (1, 2), (2, 1)]      # (x, y): the T and where it meets the frame
    rings = ro.trace(mask)
    assert sim.ring_list(rings)[0] == [(2, 0), (2, 1), (0, 1), (0, 0)]
    dense, _ = sim.dense_rings(rings, mask)
    assert dense[0] == [(2, 0), (2, 1), (1, 1), (0, 1), (0, 0)], "the node follows the vertex whose run it lies on"
    assert sim.anchor_positions(dense[0], node) == [1, 2, 3]
    for tolerance in (0, 1.5, 1000):      # anchors stay, the frame's corners go once the tolerance reaches them
        out = _simplified(mask, tolerance)
        assert out[0] == ([(2, 0), (2, 1), (1, 1), (0, 1), (0, 0)] if tolerance < 1 else [(2, 1), (1, 1), (0, 1)]), tolerance
    # with values=[1] the other cells are one class: no node, a free ring from its smallest vertex
    assert not sim.nodes(mask, values=[1]).any()
    assert _simplified(mask, 0, values=[1]) == [[(2, 0), (2, 1), (0, 1), (0, 0)]]
    assert _simplified(mask, 1000, values=[1]) == [[(0, 0)]]


def test_a_checkerboard_has_a_degree_4_node():
    mask = _rows("01", "10")
    node = sim.nodes(mask)
    assert node[1, 1] == 1 and node.sum() == 5 and not node[0, 0]
    for connectivity in (4, 8):      # nodes do not depend on the connectivity
        for tolerance in (0, 1000):
            out = _simplified(mask, tolerance, connectivity=connectivity)
            corners = {(0, 0), (2, 0), (0, 2), (2, 2)}
            assert all((1, 1) in ring for ring in out)
            assert any(corners & set(ring) for ring in out) == (tolerance == 0), "only the frame's corners are no nodes"


def test_a_free_island_collapses_with_the_hole_it_sits_in():
    mask = np.zeros((7, 9), dtype=np.uint8)
    mask[2:4, 3:7] = 1      # 4 wide, 2 high, no node anywhere
    assert not sim.nodes(mask).any()
    hole, island = [(3, 2), (3, 4), (7, 4), (7, 2)], [(7, 2), (7, 4), (3, 4), (3, 2)]      # the hole starts a pixel row earlier
    frame = [(9, 0), (9, 7), (0, 7), (0, 0)]
    assert _simplified(mask, 0) == [frame, hole, island]
    assert _simplified(mask, 1.5) == [frame, hole, island], "below its width: the far corner splits, the other two are 1.79 away"
    # above its width but below its diagonal: the anchor (3, 2) and the farthest vertex (7, 4) stay, in both rings
    assert _simplified(mask, 2) == [frame, [(3, 2), (7, 4)], [(7, 4), (3, 2)]]
    assert _simplified(mask, 5) == [frame, [(3, 2)], [(3, 2)]], "above the diagonal (4.47): the anchor alone, in both"
    assert _simplified(mask, 12) == [[(0, 0)], [(3, 2)], [(3, 2)]]


def test_a_staircase_reduces_to_its_two_ends():
    n = 12
    y, x = np.mgrid[0:n, 0:n]
    mask = (x > y).astype(np.uint8)      # the diagonal staircase between two regions, both on the frame
    lower = _simplified(mask, 0.75)[0]
    assert (1, 0) in lower and (n, n - 1) in lower, "the nodes where the staircase meets the frame"
    assert [p for p in lower if 0 < p[0] < n and 0 < p[1] < n] == [], "every step lies within 0.71 of the chord"
    assert lower == [(1, 0), (12, 11), (12, 12), (0, 12), (0, 0)]
    fine = _simplified(mask, 0.5)[0]
    assert (1, 1) in fine, "the first step is 0.707 from the chord: it stays below that tolerance"


# ------------------------------------------------------------------ the oracle's invariants on the patterns
@functools.lru_cache(maxsize=None)
def _case(name: str, connectivity: int, ignore: int, rim: bool):
    mask = PATTERNS[name][0](*SHAPE)
    if rim:
        mask = np.pad(mask, 1, constant_values=RIM)
    rings = ro.trace(mask, connectivity, ignore)
    return mask, rings, sim.dense_rings(rings, mask, ignore)


def _cases():
    return [(name, c, ign) for name in PATTERNS for c in (4, 8) for ign in (-1, PATTERNS[name][1])]


@pytest.mark.parametrize("name,connectivity,ignore", _cases(), ids=lambda v: str(v))
def test_dense_rings_and_dropped_vertices(name, connectivity, ignore):
    mask, rings, (dense, node) = _case(name, connectivity, ignore, False)
    for ring, d in zip(sim.ring_list(rings), dense):      # (a) without the nodes it runs straight through, a dense ring is the ring
        turns = [q for p, q, r in zip(d[-1:] + d[:-1], d, d[1:] + d[:1]) if (q[0] - p[0]) * (r[1] - q[1]) != (q[1] - p[1]) * (r[0] - q[0])]
        assert turns == ring
        assert all(node[y, x] for x, y in set(d) - set(ring)), "only nodes are inserted"
        loose = [p for p in d if not node[p[1], p[0]]]
        assert len(set(loose)) == len(loose), "no lattice point occurs twice among the non-anchor vertices"
    for tolerance in TOLERANCES:      # (b) a dropped vertex lies within the tolerance of the chord of the segment it ended in
        q = sim.quantise(tolerance)
        for d in dense:
            trail = []
            kept, _ = sim.simplify_ring(d, sim.anchor_positions(d, node), q, trail)
            dropped = [k for _, _, ks in trail for k in ks]
            assert sorted(dropped + kept) == list(range(len(d))), "every vertex is kept or dropped once"
            for i, j, ks in trail:
                (ax, ay), (bx, by) = d[i], d[j]
                for k in ks:
                    px, py = d[k]
                    if (ax, ay) == (bx, by):
                        assert ((px - ax) ** 2 + (py - ay) ** 2) * 2 ** 16 <= q * q
                    else:
                        cross = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
                        assert cross * cross * 2 ** 16 <= q * q * ((bx - ax) ** 2 + (by - ay) ** 2)


def shared_boundary(rings, tolerance: float) -> None:
    """(c) on simplified rings of a mask with a rim; see the module docstring for what holds at which tolerance."""
    rl = sim.ring_list(rings)
    count = Counter((a, b) for ring in rl[1:] if len(ring) > 1 for a, b in zip(ring, ring[1:] + ring[:1]))
    for (a, b), n in count.items():
        assert count[b, a] == n, ("a segment and its reverse occur equally often", a, b, tolerance)
    if tolerance == 0:
        assert set(count.values()) <= {1}, "nothing collapses at tolerance 0: every directed segment occurs exactly once"


@pytest.mark.parametrize("name", list(PATTERNS))
def test_neighbours_share_their_simplified_boundary(name):
    for connectivity in (4, 8):
        mask, rings, dense = _case(name, connectivity, -1, True)
        assert rings.start[0] == 0 and rings.value[0] == RIM and rings.area2[0] == 2 * mask.size, "ring 0 is the frame"
        for tolerance in TOLERANCES:
            out, _ = sim.simplify(rings, mask, sim.quantise(tolerance), dense=dense)
            shared_boundary(out, tolerance)
