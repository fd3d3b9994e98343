"""The sieve of include/gdlhip_scene_sieve.h restated in numpy and plain Python, the yardstick of tests/test_scene_sieve_host.py and
tests/test_hip_scene_sieve.py, with the masks both files try it on.

``components``: a union-find over the pixels in raster order that always hangs the larger root under the smaller, so a
component's root is its smallest linear index.  ``sieve_once``: the key ``(size << 8) | (255 - value)`` of every kept component
next to a pixel of a small one, maximised per small root; ``sieve`` repeats the two."""

import numpy as np


def _pairs(connectivity: int):
    """(dy, dx) of half the neighbourhood: with the opposite steps, all of it."""
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity {connectivity}")
    return [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])


def _views(a: np.ndarray, dy: int, dx: int):
    """(a at p, a at p + (dy, dx)) over every p for which both lie inside; dy >= 0."""
    H, W = a.shape
    if dx >= 0:
        return a[:H - dy, :W - dx], a[dy:, dx:]
    return a[:H - dy, -dx:], a[dy:, :W + dx]


def components(mask: np.ndarray, connectivity: int = 4, ignore_label: int = -1):
    """(labels int32 [H, W], sizes int32 [H*W]): the smallest linear index of the pixel's component (-1 where the pixel equals
    ``ignore_label``), and at that index the component's pixel count (0 at every other index)."""
    H, W = mask.shape
    index = np.arange(H * W).reshape(H, W)
    parent = list(range(H * W))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    live = mask != ignore_label
    for dy, dx in _pairs(connectivity):
        (ma, mb), (la, lb), (ia, ib) = _views(mask, dy, dx), _views(live, dy, dx), _views(index, dy, dx)
        joined = (ma == mb) & la & lb
        for a, b in zip(ia[joined].tolist(), ib[joined].tolist()):
            a, b = find(a), find(b)
            if a != b:
                parent[max(a, b)] = min(a, b)
    labels = np.array([find(i) for i in range(H * W)], dtype=np.int32).reshape(H, W)
    labels[~live] = -1
    sizes = np.bincount(labels[live], minlength=H * W).astype(np.int32)
    return labels, sizes


def sieve_once(mask: np.ndarray, min_size: int, connectivity: int = 4, ignore_label: int = -1, comps=None) -> np.ndarray:
    H, W = mask.shape
    labels, sizes = comps if comps is not None else components(mask, connectivity, ignore_label)
    size_of = np.where(labels >= 0, sizes[np.maximum(labels, 0)], 0).astype(np.int64)      # of the pixel's component; 0: ignored
    small, kept = (labels >= 0) & (size_of < min_size), (labels >= 0) & (size_of >= min_size)
    key = (size_of << 8) | (255 - mask.astype(np.int64))
    best = np.zeros(H * W, dtype=np.int64)
    for dy, dx in _pairs(connectivity):
        for a, b in ((0, 1), (1, 0)):      # the step and its opposite
            s, k, lab, ky = (_views(v, dy, dx) for v in (small, kept, labels, key))
            hit = s[a] & k[b]      # a kept neighbour is another component: a small and a kept one never share a label
            np.maximum.at(best, lab[a][hit], ky[b][hit])
    won = best[np.maximum(labels, 0)]
    return np.where(small & (won > 0), 255 - (won & 255), mask).astype(np.uint8)


def sieve(mask: np.ndarray, min_size: int, connectivity: int = 4, ignore_label: int = -1, iterations: int = 1, comps=None) -> np.ndarray:
    """``comps``: what ``components`` gives for ``mask``, where the caller has it already."""
    for _ in range(iterations):
        mask, comps = sieve_once(mask, min_size, connectivity, ignore_label, comps), None
    return mask


# ------------------------------------------------------------------ masks
def spiral(H: int, W: int) -> np.ndarray:
    """One arm of 1s, one pixel wide, wound inwards with a gap of one pixel: ring k = 0, 2, 4, ... runs along the top, right and
    bottom of the rectangle inset by k and up its left side to two rows below the top, where the next ring's top row takes over."""
    m = np.zeros((H, W), dtype=np.uint8)
    for k in range(0, (min(H, W) + 1) // 2, 2):
        top, bottom, left, right = k, H - 1 - k, k, W - 1 - k
        m[top, max(left - 1, 0):right + 1] = 1
        m[top:bottom + 1, right] = 1
        if bottom > top:
            m[bottom, left:right + 1] = 1
        if right > left:
            m[top + 2:bottom + 1, left] = 1
    return m


def _grid(H: int, W: int):
    return np.mgrid[0:H, 0:W]


def _random(H: int, W: int, seed: int, classes: int = 2, p: float | None = None) -> np.ndarray:
    g = np.random.default_rng([seed, H, W])
    if p is not None:
        return (g.random((H, W)) < p).astype(np.uint8)
    return g.integers(0, classes, (H, W)).astype(np.uint8)


def _comb(H: int, W: int) -> np.ndarray:
    m = np.zeros((H, W), dtype=np.uint8)
    m[0, :] = 1
    m[:, ::2] = 1
    return m


def _rings(H: int, W: int) -> np.ndarray:
    y, x = _grid(H, W)
    return (np.minimum(np.minimum(y, H - 1 - y), np.minimum(x, W - 1 - x)) % 2).astype(np.uint8)


def _cross(H: int, W: int, tile: int) -> np.ndarray:
    """Three classes at random, cut by a cross of 255: its row is the first row of the second tile row and its column the last
    column of the first tile column (the middle row / column where the mask is smaller than that)."""
    m = _random(H, W, 5, classes=3)
    m[tile if H > tile else H // 2, :] = 255
    m[:, tile - 1 if W >= tile else W // 2] = 255
    return m


# name -> (mask(H, W), the ignore_label it is also tried with); `tile` is the edge of the kernels' tile
def patterns(tile: int = 64) -> dict:
    return {
        "spiral": (spiral, 1),
        "checkerboard": (lambda H, W: (np.add(*_grid(H, W)) % 2).astype(np.uint8), 1),
        "diagonal-lines": (lambda H, W: (np.add(*_grid(H, W)) % 4 == 0).astype(np.uint8), 1),
        "diagonal-bands": (lambda H, W: (np.add(*_grid(H, W)) // 3 % 3).astype(np.uint8), 1),
        "comb": (_comb, 1),
        "rings": (_rings, 1),
        "constant": (lambda H, W: np.full((H, W), 7, dtype=np.uint8), 7),
        "random-2": (lambda H, W: _random(H, W, 2), 1),
        "random-5": (lambda H, W: _random(H, W, 3, classes=5), 1),
        "percolation": (lambda H, W: _random(H, W, 4, p=0.5927), 1),      # the site threshold of the square lattice
        "ignore-cross": (lambda H, W: _cross(H, W, tile), 255),
    }


# ------------------------------------------------------------------ hand-drawn 5 x 7 cases
def _rows(*rows: str) -> np.ndarray:
    return np.array([[int(c) for c in r] for r in rows], dtype=np.uint8)


# (name, mask, keyword arguments, the expected result); a 9 is the ignore_label where one is given
HAND_CASES = [
    ("the larger neighbour wins over the lower class",      # 19 pixels of 1 against 15 of 0
     _rows("1111000", "1111000", "1112000", "1111000", "1111000"), dict(min_size=3),
     _rows("1111000", "1111000", "1111000", "1111000", "1111000")),
    ("equal sizes give the lower class",      # 15 pixels each side of the column of 5
     _rows("3335111", "3335111", "3335111", "3335111", "3335111"), dict(min_size=6),
     _rows("3331111", "3331111", "3331111", "3331111", "3331111")),
    ("fenced in by ignore_label: unchanged, while the free one goes",
     _rows("0000001", "0099900", "0092900", "0099900", "0000000"), dict(min_size=4, ignore_label=9),
     _rows("0000000", "0099900", "0092900", "0099900", "0000000")),
    ("fenced in, connectivity 8",
     _rows("0000001", "0099900", "0092900", "0099900", "0000000"), dict(min_size=4, ignore_label=9, connectivity=8),
     _rows("0000000", "0099900", "0092900", "0099900", "0000000")),
    ("touching small regions only: unchanged in one pass",
     _rows("0000000", "0001000", "0012100", "0001000", "0000000"), dict(min_size=2),
     _rows("0000000", "0000000", "0002000", "0000000", "0000000")),
    ("touching small regions only: absorbed in the second pass",
     _rows("0000000", "0001000", "0012100", "0001000", "0000000"), dict(min_size=2, iterations=2),
     _rows("0000000", "0000000", "0000000", "0000000", "0000000")),
    ("two blocks across a diagonal, connectivity 4: two regions of 4",
     _rows("1100000", "1100000", "0011000", "0011000", "0000000"), dict(min_size=5, connectivity=4),
     _rows("0000000", "0000000", "0000000", "0000000", "0000000")),
    ("two blocks across a diagonal, connectivity 8: one region of 8",
     _rows("1100000", "1100000", "0011000", "0011000", "0000000"), dict(min_size=5, connectivity=8),
     _rows("1100000", "1100000", "0011000", "0011000", "0000000")),
    ("no kept region at all: unchanged",
     _rows("1100000", "1100000", "0011000", "0011000", "0000000"), dict(min_size=36),
     _rows("1100000", "1100000", "0011000", "0011000", "0000000")),
]
