"""The per-region attributes of include/gdlhip_scene_regions.h restated in numpy, the yardstick of
tests/test_scene_regions_host.py and tests/test_hip_scene_regions.py, with cases whose seven results are written out by hand.

``regions``: the labels are those of ``_sieve_oracle.components``; the regions are numbered by ascending label, counts and sums
come from ``np.bincount`` / ``np.add.at`` and the box and the lowest confidence from ``np.minimum.at`` / ``np.maximum.at``.
``confidence``: the pixel's q from f32 probabilities [K, H, W] and the weight plane, every step in ``np.float32``."""

from typing import NamedTuple

import numpy as np

from _sieve_oracle import components

I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


class Regions(NamedTuple):
    label: np.ndarray         # int32 [N]
    value: np.ndarray         # uint8 [N]
    pixels: np.ndarray        # int32 [N]
    bbox: np.ndarray          # int32 [N, 4]: x0, y0, x1, y1, the last two exclusive
    sum_xy: np.ndarray        # int64 [N, 2]
    conf_sum: np.ndarray      # int64 [N], None without probabilities
    conf_min: np.ndarray      # int32 [N], None without probabilities


def confidence(mask: np.ndarray, probs: np.ndarray, weight: np.ndarray) -> np.ndarray:
    """q (int32 [H, W]) of every pixel: rint(65536 p) with p the probability of the pixel's own class -- probs[v] for K >= 2;
    for K == 1 probs[0] where v is 1 and 1 - probs[0] where v is 0 -- and 0 where the weight is 0 or there is no plane for v."""
    assert probs.dtype == np.float32 and probs.ndim == 3 and probs.shape[1:] == mask.shape == weight.shape
    K = probs.shape[0]
    v = mask.astype(np.int64)
    has = v <= 1 if K == 1 else v < K
    plane = np.zeros_like(v) if K == 1 else np.minimum(v, K - 1)
    p = np.take_along_axis(probs, plane[None], axis=0)[0]
    if K == 1:
        p = np.where(v == 0, np.float32(1.0) - p, p)
    assert p.dtype == np.float32
    q = np.rint(p * np.float32(65536.0)).astype(np.int32)
    return np.where(has & (weight != 0), q, 0).astype(np.int32)


def regions(mask: np.ndarray, labels: np.ndarray, probs: np.ndarray | None = None, weight: np.ndarray | None = None) -> Regions:
    """``labels``: what ``components(mask, connectivity, ignore_label)`` gives.  ``probs`` f32 [K, H, W] and ``weight`` f32 [H, W]
    come together or not at all."""
    assert (probs is None) == (weight is None)
    live = labels >= 0
    roots = np.unique(labels[live]).astype(np.int32)      # ascending
    N = len(roots)
    number = np.searchsorted(roots, labels[live])         # the region of every live pixel, in raster order
    y, x = np.nonzero(live)                               # the same order
    pixels = np.bincount(number, minlength=N).astype(np.int32)
    value = mask.reshape(-1)[roots].astype(np.uint8)
    bbox = np.empty((N, 4), dtype=np.int32)
    bbox[:, :2], bbox[:, 2:] = I32_MAX, I32_MIN
    np.minimum.at(bbox[:, 0], number, x)
    np.minimum.at(bbox[:, 1], number, y)
    np.maximum.at(bbox[:, 2], number, x + 1)
    np.maximum.at(bbox[:, 3], number, y + 1)
    sum_xy = np.zeros((N, 2), dtype=np.int64)
    np.add.at(sum_xy[:, 0], number, x)
    np.add.at(sum_xy[:, 1], number, y)
    conf_sum = conf_min = None
    if probs is not None:
        q = confidence(mask, probs, weight)[live]
        conf_sum, conf_min = np.zeros(N, dtype=np.int64), np.full(N, I32_MAX, dtype=np.int32)
        np.add.at(conf_sum, number, q)
        np.minimum.at(conf_min, number, q)
    return Regions(roots, value, pixels, bbox, sum_xy, conf_sum, conf_min)


def of_mask(mask: np.ndarray, connectivity: int = 4, ignore_label: int = -1, probs=None, weight=None) -> Regions:
    return regions(mask, components(mask, connectivity, ignore_label)[0], probs, weight)


def tile_label_counts(labels: np.ndarray, tile: int) -> np.ndarray:
    """The number of distinct labels (>= 0) in every tile x tile square of the raster, row-major."""
    H, W = labels.shape
    return np.array([len(np.unique(t[t >= 0])) for y in range(0, H, tile) for x in range(0, W, tile)
                     for t in [labels[y:y + tile, x:x + tile]]])


# ------------------------------------------------------------------ cases written out by hand
def _rows(*rows: str) -> np.ndarray:
    return np.array([[int(c) for c in r] for r in rows], dtype=np.uint8)


def _f32(rows) -> np.ndarray:
    return np.array(rows, dtype=np.float32)


def _want(label, value, pixels, bbox, sum_xy, conf_sum=None, conf_min=None) -> Regions:
    return Regions(np.array(label, dtype=np.int32), np.array(value, dtype=np.uint8), np.array(pixels, dtype=np.int32),
                   np.array(bbox, dtype=np.int32).reshape(-1, 4), np.array(sum_xy, dtype=np.int64).reshape(-1, 2),
                   None if conf_sum is None else np.array(conf_sum, dtype=np.int64),
                   None if conf_min is None else np.array(conf_min, dtype=np.int32))


# every probability below is a multiple of 1 / 4, so q is one of 0, 16384, 32768, 49152, 65536
_RING_P1 = _f32([[0.5, 0.75, 0.75, 0.75]] + [[0.75] * 4] * 3)
_DIAG_P1 = _f32([[1.0, 0.25], [0.5, 0.5]])
_ONES = lambda *shape: np.ones(shape, dtype=np.float32)      # noqa: E731

# (name, mask, dict(connectivity=, ignore_label=), probs or None, weight or None, the seven results)
HAND_CASES = [
    ("a region with a hole",      # the rim of 12 ones is label 0, the 2 x 2 hole of zeros label 5; the rim's corner pixel is less sure
     _rows("1111", "1001", "1001", "1111"), dict(connectivity=4), np.stack([1 - _RING_P1, _RING_P1]), _ONES(4, 4),
     _want([0, 5], [1, 0], [12, 4], [[0, 0, 4, 4], [1, 1, 3, 3]], [[18, 18], [6, 6]], [11 * 49152 + 32768, 4 * 16384], [32768, 16384])),
    ("two diagonal pixels, connectivity 4: four regions",
     _rows("10", "01"), dict(connectivity=4), np.stack([1 - _DIAG_P1, _DIAG_P1]), _ONES(2, 2),
     _want([0, 1, 2, 3], [1, 0, 0, 1], [1, 1, 1, 1], [[0, 0, 1, 1], [1, 0, 2, 1], [0, 1, 1, 2], [1, 1, 2, 2]],
           [[0, 0], [1, 0], [0, 1], [1, 1]], [65536, 49152, 32768, 32768], [65536, 49152, 32768, 32768])),
    ("two diagonal pixels, connectivity 8: two regions over the same box",
     _rows("10", "01"), dict(connectivity=8), np.stack([1 - _DIAG_P1, _DIAG_P1]), _ONES(2, 2),
     _want([0, 1], [1, 0], [2, 2], [[0, 0, 2, 2], [0, 0, 2, 2]], [[1, 1], [1, 1]], [65536 + 32768, 49152 + 32768], [32768, 32768])),
    ("an ignored stripe, no canvas",      # column 2 is ignore_label 9: one class on both sides, two regions
     _rows("2292", "2292", "2292"), dict(connectivity=8, ignore_label=9), None, None,
     _want([0, 3], [2, 2], [6, 3], [[0, 0, 2, 3], [3, 0, 4, 3]], [[3, 6], [9, 3]])),
    ("one class (K = 1), both values, an uncovered pixel",      # pixel (1, 2) has weight 0: q = 0 although v = 0 and 1 - 0 = 1
     _rows("110", "100"), dict(connectivity=4), _f32([[[0.75, 1.0, 0.25], [0.5, 0.25, 0.0]]]), _f32([[1, 1, 1], [1, 1, 0]]),
     _want([0, 2], [1, 0], [3, 3], [[0, 0, 2, 2], [1, 0, 3, 2]], [[1, 1], [5, 2]], [49152 + 65536 + 32768, 49152 + 49152 + 0], [32768, 0])),
    ("a mask value the canvas has no plane for (K = 2)",
     _rows("051"), dict(connectivity=4), _f32([[[0.5, 0.5, 0.25]], [[0.5, 0.5, 0.75]]]), _ONES(1, 3),
     _want([0, 1, 2], [0, 5, 1], [1, 1, 1], [[0, 0, 1, 1], [1, 0, 2, 1], [2, 0, 3, 1]], [[0, 0], [1, 0], [2, 0]], [32768, 0, 49152],
           [32768, 0, 49152])),
    ("a mask value above 1 with one class (K = 1)",
     _rows("21"), dict(connectivity=4), _f32([[[0.5, 0.5]]]), _ONES(1, 2),
     _want([0, 1], [2, 1], [1, 1], [[0, 0, 1, 1], [1, 0, 2, 1]], [[0, 0], [1, 0]], [0, 32768], [0, 32768])),
]


def same(got, want) -> bool:
    """Whether two sets of seven results are equal field for field, types included."""
    for g, w in zip(got, want):
        if (g is None) != (w is None):
            return False
        if g is not None and not (g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)):
            return False
    return True
