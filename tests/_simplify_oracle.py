"""The ring simplification of include/gdlhip_scene_simplify.h restated in numpy and plain Python, the yardstick of
tests/test_scene_simplify_host.py and tests/test_hip_scene_simplify.py.  It builds on tests/_rings_oracle.py for the input rings.

``nodes``: the node plane from the classes of the four cells around every lattice point.  ``densify``: every ring walked run by
run, the nodes strictly inside a run inserted behind the run's first vertex.  ``anchor_positions``: the positions of a dense
ring's nodes, or of its smallest (y, x) vertex where it has none.  ``simplify``: Douglas-Peucker with an explicit stack over
every arc between two anchors, the measures as int64 arrays (they stay below 2^58), the test with Python integers; it returns the
simplified rings and the largest depth reached, where an arc has depth 1 and the two halves of a split segment one more than the
segment: the number of rounds the device needs, each of which handles every segment of one depth."""

import numpy as np

import _rings_oracle as ro

TOL_MAX = 2 ** 20


def quantise(tolerance: float) -> int:
    """tol_q8 = round(tolerance * 256)."""
    if not 0 <= tolerance <= TOL_MAX:
        raise ValueError(f"tolerance {tolerance}")
    return int(round(tolerance * 256))


def classes(mask: np.ndarray, ignore_label: int = -1, values=None) -> np.ndarray:
    """int16 [H + 2, W + 2]: the class of every cell of the raster and of a rim of cells around it (256: not live)."""
    H, W = mask.shape
    padded = np.full((H + 2, W + 2), 256, dtype=np.int16)
    padded[1:-1, 1:-1] = np.where(ro.live_pixels(mask, ignore_label, values), mask.astype(np.int16), np.int16(256))
    return padded


def nodes(mask: np.ndarray, ignore_label: int = -1, values=None) -> np.ndarray:
    """uint8 [H + 1, W + 1]: 1 where at least 3 of the 4 unit lattice edges at (x, y) separate two classes."""
    c = classes(mask, ignore_label, values)
    nw, ne, sw, se = c[:-1, :-1], c[:-1, 1:], c[1:, :-1], c[1:, 1:]      # the cells around lattice point (x, y)
    degree = (nw != ne).astype(np.int8) + (sw != se) + (nw != sw) + (ne != se)
    return (degree >= 3).astype(np.uint8)


def ring_list(rings) -> list:
    """The rings as lists of (x, y) tuples of Python ints."""
    v, off = np.asarray(rings.vertices).tolist(), np.asarray(rings.ring_offsets).tolist()
    return [[(x, y) for x, y in v[off[r]:off[r + 1]]] for r in range(len(off) - 1)]


def densify(ring: list, node: np.ndarray) -> list:
    """The dense ring: the nodes strictly inside a straight run follow the run's first vertex, in the order of travel."""
    dense = []
    for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1]):
        dense.append((x0, y0))
        if (x0 == x1) == (y0 == y1):
            raise ValueError(f"the run {(x0, y0)} -> {(x1, y1)} is not axis-parallel")
        dx, dy = (x1 > x0) - (x1 < x0), (y1 > y0) - (y1 < y0)
        for t in range(1, abs(x1 - x0) + abs(y1 - y0)):
            if node[y0 + t * dy, x0 + t * dx]:
                dense.append((x0 + t * dx, y0 + t * dy))
    return dense


def anchor_positions(dense: list, node: np.ndarray) -> list:
    at = [i for i, (x, y) in enumerate(dense) if node[y, x]]
    return at or [min(range(len(dense)), key=lambda i: (dense[i][1], dense[i][0]))]


def passes(measure: int, closed: bool, d2: int, tol_q8: int) -> bool:
    """c^2 * 2^16 > tol_q8^2 * |b - a|^2, or |p - a|^2 * 2^16 > tol_q8^2, with Python integers."""
    return measure * 2 ** 16 > tol_q8 ** 2 if closed else measure ** 2 * 2 ** 16 > tol_q8 ** 2 * d2


def douglas_peucker(points: np.ndarray, tol_q8: int, trail=None) -> tuple[list, int]:
    """``points``: int64 [n, 2], an arc from points[0] to points[-1].  (the kept positions 0 .. n - 1 ascending, the depth).
    ``trail``: a list that takes, for every segment that kept nothing, (its two end positions, the positions it dropped)."""
    n, kept, depth = len(points), [0, len(points) - 1], 1
    stack = [(0, n - 1, 1)]
    while stack:
        i, j, level = stack.pop()
        if j - i < 2:
            continue
        depth = max(depth, level)
        a, b, p = points[i], points[j], points[i + 1:j]
        closed = bool((a == b).all())
        if closed:
            measure = ((p - a) ** 2).sum(axis=1)
        else:
            measure = np.abs((b[0] - a[0]) * (p[:, 1] - a[1]) - (b[1] - a[1]) * (p[:, 0] - a[0]))
        best = np.flatnonzero(measure == measure.max())
        w = int(best[np.lexsort((p[best, 0], p[best, 1]))[0]])      # of equal ones the smallest (y, x)
        if passes(int(measure[w]), closed, int(((b - a) ** 2).sum()), tol_q8):
            kept.append(i + 1 + w)
            stack += [(i, i + 1 + w, level + 1), (i + 1 + w, j, level + 1)]
        elif trail is not None:
            trail.append((i, j, list(range(i + 1, j))))
    return sorted(kept), depth


def simplify_ring(dense: list, anchors: list, tol_q8: int, trail=None) -> tuple[list, int]:
    """(the kept positions of the dense ring ascending, the depth).  ``trail`` as in ``douglas_peucker``, the positions the
    dense ring's (taken modulo its length)."""
    n, kept, depth = len(dense), set(anchors), 1
    for s, e in zip(anchors, anchors[1:] + [anchors[0] + n]):      # cyclically; a single anchor: one closed arc
        arc = np.array([dense[i % n] for i in range(s, e + 1)], dtype=np.int64)
        local = [] if trail is not None else None
        positions, d = douglas_peucker(arc, tol_q8, local)
        kept.update((s + i) % n for i in positions)
        depth = max(depth, d)
        if trail is not None:
            trail += [((s + i) % n, (s + j) % n, [(s + k) % n for k in dropped]) for i, j, dropped in local]
    return sorted(kept), depth


def dense_rings(rings, mask: np.ndarray, ignore_label: int = -1, values=None) -> tuple[list, np.ndarray]:
    """(the dense rings as lists of (x, y), the node plane)."""
    node = nodes(mask, ignore_label, values)
    return [densify(ring, node) for ring in ring_list(rings)], node


def simplify(rings, mask: np.ndarray, tol_q8: int, ignore_label: int = -1, values=None, dense=None) -> tuple[ro.Rings, int]:
    """(the simplified rings, the largest depth).  ``dense``: what ``dense_rings`` gave for the same arguments, where the caller
    has it (it does not depend on the tolerance)."""
    dense, node = dense if dense is not None else dense_rings(rings, mask, ignore_label, values)
    vertices, offsets, depth = [], [0], 0
    for ring in dense:
        kept, d = simplify_ring(ring, anchor_positions(ring, node), tol_q8)
        vertices += [ring[i] for i in kept]
        offsets.append(len(vertices))
        depth = max(depth, d)
    out = ro.Rings(np.array(vertices, dtype=np.int32).reshape(-1, 2), np.array(offsets, dtype=np.int32), rings.value, rings.label,
                   rings.start, rings.area2)
    return out, depth
