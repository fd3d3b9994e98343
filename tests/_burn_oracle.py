"""The burn rule of include/gdlhip_scene_burn.h restated in Python integers and numpy, the yardstick of
tests/test_scene_burn_host.py and tests/test_hip_scene_burn.py.  It shares no code with the library.

``crossings``: the list of (y, x0, w, value) of every edge of every ring, by the header's integer quotient.  ``burn``: the two
difference planes those add up to, their sums along the rows, and the resolved raster with its counts.  ``bad_entries``: what
gdl_scene_burn_count counts as bad.  ``fan``: a random triangulation of a rectangle in 1 / 256 pixel.  ``HAND_CASES``: small inputs whose results are written out by hand."""

from typing import NamedTuple

import numpy as np


class Burn(NamedTuple):      # the fields of gdlhip.ops.SceneBurn
    mask: np.ndarray          # uint8 [H, W]
    conflicts: int
    differ: object            # int, or None without a reference


class Rings(NamedTuple):      # what ops.scene_burn reads of a SceneRings
    vertices: np.ndarray      # int32 [V, 2]
    ring_offsets: np.ndarray  # int32 [R + 1]
    value: np.ndarray         # uint8 [R]


def make(rings, scale: int = 1) -> Rings:
    """Rings of [(value, [(x, y), ...]), ...], every coordinate times ``scale``."""
    vertices = [(x * scale, y * scale) for _, ring in rings for x, y in ring]
    offsets = np.cumsum([0] + [len(ring) for _, ring in rings])
    return Rings(np.array(vertices, dtype=np.int32).reshape(-1, 2), offsets.astype(np.int32), np.array([v for v, _ in rings], dtype=np.uint8))


def _ceil(a: int, b: int) -> int:
    return -((-a) // b)


def crossings(rings, H: int, W: int, bits: int = 0) -> list:
    u = 1 << bits
    vertices, offsets, value = (np.asarray(f).tolist() for f in (rings.vertices, rings.ring_offsets, rings.value))
    found = []
    for r in range(len(offsets) - 1):
        ring = vertices[offsets[r]:offsets[r + 1]]
        if len(ring) < 3:
            continue
        for (ax, ay), (bx, by) in zip(ring, ring[1:] + ring[:1]):
            ax, ay, bx, by = 2 * ax, 2 * ay, 2 * bx, 2 * by
            dy, dx = by - ay, bx - ax
            if dy == 0:
                continue
            # the rows with min(ay, by) <= (2 y + 1) u < max(ay, by)
            first, end = max(0, _ceil(min(ay, by) - u, 2 * u)), min(H, _ceil(max(ay, by) - u, 2 * u))
            for y in range(first, end):
                cy = (2 * y + 1) * u
                assert min(ay, by) <= cy < max(ay, by)
                sign = 1 if dy > 0 else -1
                P = sign * (ax * dy + (cy - ay) * dx)
                x0 = _ceil(P - abs(dy) * u, 2 * abs(dy) * u)
                if x0 < W:
                    found.append((y, max(x0, 0), 1 if dy < 0 else -1, value[r]))
    return found


def burn(rings, H: int, W: int, bits: int = 0, background: int = 0, conflict: int = 255, reference=None) -> Burn:
    C, S = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    found = crossings(rings, H, W, bits)
    if found:
        y, x, w, v = np.array(found, dtype=np.int64).T
        np.add.at(C, (y, x), w)
        np.add.at(S, (y, x), w * v)
    C, S = np.cumsum(C, axis=1), np.cumsum(S, axis=1)
    inside, outside = (C == 1) & (S >= 0) & (S <= 255), (C == 0) & (S == 0)
    mask = np.where(inside, S, np.where(outside, background, conflict)).astype(np.uint8)
    differ = None if reference is None else int((mask != np.asarray(reference).astype(np.uint8)).sum())
    return Burn(mask, int((~inside & ~outside).sum()), differ)


def bad_entries(rings, bits: int = 0) -> int:
    v, off = np.asarray(rings.vertices, dtype=np.int64), np.asarray(rings.ring_offsets, dtype=np.int64)
    bad_offset = (off < 0) | (off > len(v))
    bad_offset[1:] |= np.diff(off) < 0
    return int((np.abs(v) > 2 ** (20 + bits)).sum()) + int(bad_offset.sum())


def fan(H: int, W: int, seed: int) -> Rings:
    """A fan of triangles around a random point of the rectangle 0 .. W x 0 .. H, vertices in 1 / 256 pixel."""
    g = np.random.default_rng([seed, H, W])
    q = 256
    top = sorted({0, W * q, *g.integers(0, W * q, 5).tolist()})
    right = sorted({0, H * q, *g.integers(0, H * q, 5).tolist()})
    rim = [(x, 0) for x in top[:-1]] + [(W * q, y) for y in right[:-1]] + [(x, H * q) for x in top[:0:-1]] + [(0, y) for y in right[:0:-1]]
    centre = (int(g.integers(1, W * q)), int(g.integers(1, H * q)))
    return make([(int(g.integers(1, 6)), [centre, a, b]) for a, b in zip(rim, rim[1:] + rim[:1])])


def _rows(*rows: str) -> np.ndarray:
    return np.array([[int(c) for c in r] for r in rows], dtype=np.uint8)


def _square(x0: int, y0: int, x1: int, y1: int) -> list:      # region on the right hand with y down: area2 > 0
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


# (name, rings as [(value, [(x, y), ...])], bits of those coordinates, keyword arguments, expected mask, expected conflicts);
# a 9 in an expected mask is the conflict value (passed as conflict=9), an 8 the background where one is passed
HAND_CASES = [
    ("unit square", [(3, _square(1, 1, 2, 2))], 0, {}, _rows("0000", "0300", "0000"), 0),
    ("square with a hole", [(1, _square(1, 1, 5, 5)), (1, _square(2, 2, 4, 4)[::-1])], 0, dict(background=8),
     _rows("8888888", "8111188", "8188188", "8188188", "8111188", "8888888"), 0),
    ("hole with an island of another class", [(1, _square(1, 1, 5, 5)), (1, _square(2, 2, 4, 4)[::-1]), (2, _square(2, 2, 4, 4))], 0, {},
     _rows("0000000", "0111100", "0122100", "0122100", "0111100", "0000000"), 0),
    # the diagonal passes through the centres of the diagonal pixels: they lie right of it and go to the upper triangle alone
    ("two triangles on a diagonal", [(1, [(0, 0), (4, 0), (4, 4)]), (2, [(0, 0), (4, 4), (0, 4)])], 0, dict(conflict=9),
     _rows("1111", "2111", "2211", "2221"), 0),
    ("overlapping squares", [(1, _square(0, 0, 3, 3)), (2, _square(1, 1, 4, 4))], 0, dict(conflict=9),
     _rows("11100", "19920", "19920", "02220", "00000"), 4),
    ("a reversed ring", [(5, _square(1, 1, 2, 2)[::-1]), (4, _square(3, 0, 4, 1))], 0, dict(conflict=9), _rows("0004", "0900", "0000"), 1),
    ("a ring of two vertices", [(7, [(0, 0), (3, 3)]), (6, _square(0, 0, 1, 2)), (7, [(2, 0)])], 0, {}, _rows("600", "600", "000"), 0),
    # the left edge at x = -2 gives x0 = -2, clamped to 0; the right edge at x = 6 gives x0 = 6 >= W, dropped
    ("clipped on all four sides", [(2, _square(-2, -2, 6, 5))], 0, {}, _rows("2222", "2222", "2222"), 0),
    # |x - 2| + |y - 2| <= 3 around vertices outside the raster: the edges pass through the centres of the four corner pixels;
    # a centre on a left edge is in, one on a right edge out
    ("a diamond around the raster", [(3, [(2, -1), (5, 2), (2, 5), (-1, 2)])], 0, {}, _rows("3330", "3333", "3333", "3330"), 0),
    # half pixels: the rectangle 0.5 .. 2.5 x 0.5 .. 1.5 has its corners on pixel centres: the rows and columns are half open
    ("vertices on centre lines", [(4, _square(1, 1, 5, 3))], 1, {}, _rows("440", "000", "000"), 0),
    ("beyond the right and lower rim", [(1, _square(2, 1, 9, 9)), (2, _square(5, 5, 7, 7)), (3, _square(-3, -3, -1, -1))], 0, dict(conflict=9),
     _rows("000", "001", "001"), 0),
]
