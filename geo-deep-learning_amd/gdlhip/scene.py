"""Host side of whole-scene inference: where the tiles of a scene lie and what window weights them, and the transform codes of test-time augmentation (``tta_codes``, ``plan_tta``; the device side of
those: ``ops.scene_cut_d4`` / ``scene_blend_d4`` / ``scene_blend_lowres_d4``, include/gdlhip_scene_tta.h).  The device side is
``gdlhip.ops.scene_cut`` / ``scene_blend`` / ``scene_blend_lowres`` / ``scene_finish`` (include/gdlhip_scene.h) and, for nodata,
``scene_valid`` / ``scene_tile_valid`` / ``scene_cut_valid`` / ``scene_finish_valid`` (include/gdlhip_scene_nodata.h) and, for the sieve
of the finished mask, ``scene_components`` / ``scene_sieve`` (include/gdlhip_scene_sieve.h) and, for its polygon rings,
``scene_rings`` (include/gdlhip_scene_rings.h) and their simplification ``scene_rings_simplify``
(include/gdlhip_scene_simplify.h), which ``polygons`` here groups into features, and the regions' attributes
``scene_regions`` (include/gdlhip_scene_regions.h), which ``polygons`` adds to their properties, and, for the way back from
rings to a raster, ``scene_burn`` (include/gdlhip_scene_burn.h), for which ``rings_from_features`` here reads features; the
user-facing class is ``geo_deep_learning.tools.scene_inference.SceneInference``."""

from __future__ import annotations

import math
from typing import NamedTuple

import torch
from torch import Tensor

from .ops import byte_check


def axis_origins(length: int, tile: int, stride: int) -> list[int]:
    """Tile origins along one axis: 0 alone when the axis fits in a tile, otherwise 0, s, 2s, ... while the tile ends before the
    axis does, then the clamped origin ``length - tile`` (so the last tile ends with the axis and none reaches past it)."""
    if tile < 1 or length < 1:
        raise ValueError(f"plan_tiles: bad axis length {length} / tile {tile}")
    if not 1 <= stride <= tile:
        raise ValueError(f"plan_tiles: stride {stride} must be in 1..tile ({tile}): a larger one leaves gaps")
    if length <= tile:
        return [0]
    origins = list(range(0, length - tile, stride))      # o + tile < length
    origins.append(length - tile)
    return origins


def plan_tiles(H: int, W: int, tile: tuple[int, int], stride: tuple[int, int]) -> Tensor:
    """int32 [T, 2] of (y0, x0), row-major (all columns of the first tile row, then the next row): the grid of
    ``axis_origins`` along both axes.  Every pixel of the scene is covered by at least one tile."""
    ys, xs = axis_origins(int(H), int(tile[0]), int(stride[0])), axis_origins(int(W), int(tile[1]), int(stride[1]))
    return torch.tensor([(y, x) for y in ys for x in xs], dtype=torch.int32)


def window(n: int, kind: str = "hann") -> Tensor:
    """f32 [n] blending weights along one tile axis.  ``"hann"``: 0.5 - 0.5 cos(2 pi (i + 0.5) / n), the Hann window sampled at
    the pixel centres -- symmetric and strictly positive, so a covered pixel never has weight 0; ``"flat"``: ones."""
    if n < 1:
        raise ValueError(f"window: bad length {n}")
    if kind == "flat":
        return torch.ones(n, dtype=torch.float32)
    if kind == "hann":
        half = [0.5 - 0.5 * math.cos(2.0 * math.pi * (i + 0.5) / n) for i in range((n + 1) // 2)]
        return torch.tensor(half + half[:n // 2][::-1], dtype=torch.float64).float()      # mirrored: symmetric to the bit
    raise ValueError(f"window: unknown kind {kind!r} ('hann' or 'flat')")


def bounding_box(origins: Tensor, tile: tuple[int, int]) -> tuple[int, int, int, int]:
    """(y0, y1, x0, x1) around the tiles at ``origins`` (a host tensor)."""
    lo, hi = origins.min(dim=0).values, origins.max(dim=0).values
    return int(lo[0]), int(hi[0]) + int(tile[0]), int(lo[1]), int(hi[1]) + int(tile[1])


# ------------------------------------------------------------------ test-time augmentation (include/gdlhip_scene_tta.h)
# A transform code is 3 bits: 1 = flip x, 2 = flip y, 4 = transpose (applied first).  The eight codes are the symmetries of the
# square (the dihedral group D4); torch.rot90(x, 1) is code 6, rot90(x, 2) code 3 and rot90(x, 3) code 5.
D4 = tuple(range(8))
FLIPS = (0, 1, 2, 3)


def d4_apply(x: Tensor, g: int) -> Tensor:
    """T_g(x) on the last two dimensions, the host reference of the definition the kernels index by."""
    if not 0 <= int(g) <= 7:
        raise ValueError(f"d4_apply: a transform code is in 0..7, got {g}")
    y = x.transpose(-2, -1) if g & 4 else x
    y = y.flip(-2) if g & 2 else y
    return y.flip(-1) if g & 1 else y


def d4_inverse(g: int) -> int:
    """The code of T_g's inverse: g itself without a transpose, otherwise g with the two flip bits swapped."""
    if not 0 <= int(g) <= 7:
        raise ValueError(f"d4_inverse: a transform code is in 0..7, got {g}")
    return 4 | (g & 1) << 1 | (g >> 1 & 1) if g & 4 else int(g)


def tta_codes(tta, tile: tuple[int, int]) -> tuple[int, ...]:
    """The transform codes of one tile: ``None`` / ``"none"`` -> (0,), ``"flips"`` -> FLIPS, ``"d4"`` -> D4, or a sequence of
    distinct codes in 0..7, kept in its order.  A code that transposes needs a square tile."""
    if tta is None or isinstance(tta, str):
        named = {None: (0,), "none": (0,), "flips": FLIPS, "d4": D4}
        if tta not in named:
            raise ValueError(f"tta_codes: unknown tta {tta!r} (None, 'none', 'flips', 'd4' or a sequence of codes in 0..7)")
        codes = named[tta]
    else:
        try:
            codes = tuple(tta)
        except TypeError:
            raise ValueError(f"tta_codes: unknown tta {tta!r} (None, 'none', 'flips', 'd4' or a sequence of codes in 0..7)") from None
        if not codes or any(isinstance(g, bool) or not isinstance(g, int) or not 0 <= g <= 7 for g in codes):
            raise ValueError(f"tta_codes: a non-empty sequence of int codes in 0..7 is expected, got {tta!r}")
        if len(set(codes)) != len(codes):
            raise ValueError(f"tta_codes: a code is repeated in {codes}")
    if int(tile[0]) != int(tile[1]) and any(g & 4 for g in codes):
        raise ValueError(f"tta_codes: the codes {tuple(g for g in codes if g & 4)} transpose, which needs a square tile, not "
                         f"{int(tile[0])} x {int(tile[1])}")
    return codes


def plan_tta(plan: Tensor, codes) -> tuple[Tensor, Tensor]:
    """(origins int32 [T*G, 2], xforms int32 [T*G]) of the (tile, transform) pairs: tile-major, the G codes in the given order
    inside a tile.  That order is the order in which the blend accumulates."""
    codes = torch.tensor(tuple(codes), dtype=torch.int32)
    if plan.dim() != 2 or plan.shape[1] != 2 or codes.numel() < 1:
        raise ValueError(f"plan_tta: a plan [T, 2] and at least one code are expected, got {tuple(plan.shape)} and {codes.numel()} codes")
    return plan.to(torch.int32).repeat_interleave(codes.numel(), dim=0).contiguous(), codes.repeat(plan.shape[0])


# ------------------------------------------------------------------ polygons of the rings (include/gdlhip_scene_rings.h)
def polygons(rings, transform=None, regions=None) -> list[dict]:
    """The rings of ``ops.scene_rings`` (anything with its six fields, tensors or arrays) as GeoJSON-style features, one per
    component, ordered by label::

        {"type": "Feature", "properties": {"value": v, "label": l, "pixels": n},
         "geometry": {"type": "Polygon", "coordinates": [exterior, hole, ...]}}

    Every ring is closed (its first vertex stands at the end again); the exterior is the label's one ring with ``area2 > 0``, the
    holes follow by ascending ``start``; ``pixels`` is half the sum of the label's ``area2``.  ``transform``: None (coordinates
    stay Python ints) or six numbers (a, b, c, d, e, f) that map (x, y) to (a x + b y + c, d x + e y + f), the affine order of
    rasterio.  The rings are copied to the host once.  A label without exactly one exterior ring is a ValueError.

    Simplified rings (``ops.scene_rings_simplify``) can have collapsed to fewer than 3 vertices, which traced rings never have: a
    hole with fewer than 3 vertices is left out, and a label whose exterior has fewer than 3 vertices yields no feature (its
    holes go with it).  That is consistent: a collapsed island and the collapsed hole it sat in are the same arc, simplified to
    the same points, so the island's feature and the hole in its surroundings vanish together and the surrounding polygon covers
    the place.  ``area2`` is the pixel ring's, so exterior and hole are told apart, and ``pixels`` counted, as before the
    simplification.

    ``regions``: None (the features as above) or the ``SceneRegions`` of ``ops.scene_regions`` for the same mask (anything with
    its seven fields, tensors or arrays, copied to the host once).  Every feature's properties then gain ``bbox`` = [x0, y0, x1,
    y1] in pixel indices (x1, y1 exclusive), ``centroid`` = [(sum x + n / 2) / n, (sum y + n / 2) / n], the mean of the pixel
    centres, mapped through ``transform`` where one is given, and, where the regions carry confidences, ``confidence`` =
    conf_sum / (65536 n) and ``confidence_min`` = conf_min / 65536.  Regions and rings are matched by label: a ring label the
    regions do not have, or a region whose ``pixels`` is not the rings', is a ValueError; regions without rings (classes that
    ``values`` left out) are passed over, and a feature dropped for its collapsed exterior stays dropped."""
    vertices, offsets, value, label, start, area2 = (f.tolist() for f in (rings.vertices, rings.ring_offsets, rings.value,
                                                                           rings.label, rings.start, rings.area2))
    if len(offsets) != len(value) + 1 or not len(value) == len(label) == len(start) == len(area2) or offsets[-1] != len(vertices):
        raise ValueError(f"polygons: {len(offsets)} ring offsets, {len(value)} values and {len(vertices)} vertices do not belong together")
    if transform is not None:
        try:
            a, b, c, d, e, f = (float(t) for t in transform)
        except (TypeError, ValueError):
            raise ValueError(f"polygons: transform must be None or six numbers (a, b, c, d, e, f), got {transform!r}") from None
        vertices = [[a * x + b * y + c, d * x + e * y + f] for x, y in vertices]
    attributes = None
    if regions is not None:
        names = ("label", "pixels", "bbox", "sum_xy", "conf_sum", "conf_min")
        r_label, r_pixels, r_bbox, r_sum, r_csum, r_cmin = (None if getattr(regions, n) is None else getattr(regions, n).tolist()
                                                            for n in names)
        if not len(r_label) == len(r_pixels) == len(r_bbox) == len(r_sum) or (r_csum is None) != (r_cmin is None) \
                or (r_csum is not None and not len(r_csum) == len(r_cmin) == len(r_label)):
            raise ValueError(f"polygons: the fields of regions do not belong together ({len(r_label)} labels, {len(r_pixels)} pixel counts)")
        attributes = {lab: k for k, lab in enumerate(r_label)}
    by_label: dict[int, list[int]] = {}
    for r in sorted(range(len(value)), key=start.__getitem__):
        by_label.setdefault(label[r], []).append(r)
    features = []
    for lab in sorted(by_label):
        members = by_label[lab]
        exterior = [r for r in members if area2[r] > 0]
        if len(exterior) != 1:
            raise ValueError(f"polygons: label {lab} has {len(exterior)} exterior rings (area2 > 0), exactly one is expected")
        if offsets[exterior[0] + 1] - offsets[exterior[0]] < 3:      # collapsed by the simplification
            continue
        order = exterior + [r for r in members if area2[r] <= 0 and offsets[r + 1] - offsets[r] >= 3]
        coordinates = [vertices[offsets[r]:offsets[r + 1]] + vertices[offsets[r]:offsets[r] + 1] for r in order]
        properties = {"value": value[exterior[0]], "label": lab, "pixels": sum(area2[r] for r in members) // 2}
        if attributes is not None:
            k = attributes.get(lab)
            if k is None:
                raise ValueError(f"polygons: the rings have label {lab}, the regions do not: they are not those of one mask")
            n = r_pixels[k]
            if n != properties["pixels"]:
                raise ValueError(f"polygons: label {lab} has {properties['pixels']} pixels by its rings and {n} by the regions")
            cx, cy = (r_sum[k][0] + n / 2) / n, (r_sum[k][1] + n / 2) / n
            if transform is not None:
                cx, cy = a * cx + b * cy + c, d * cx + e * cy + f
            properties["bbox"], properties["centroid"] = list(r_bbox[k]), [cx, cy]
            if r_csum is not None:
                properties["confidence"], properties["confidence_min"] = r_csum[k] / (65536 * n), r_cmin[k] / 65536
        features.append({"type": "Feature", "properties": properties, "geometry": {"type": "Polygon", "coordinates": coordinates}})
    return features


# ------------------------------------------------------------------ rings of features (include/gdlhip_scene_burn.h)
class FeatureRings(NamedTuple):
    """What ``ops.scene_burn`` burns, on the host until ``.to(device)``."""

    vertices: Tensor          # int32 [V, 2]: (x, y) in units of 1 / 2^bits pixel, ring after ring, every ring open
    ring_offsets: Tensor      # int32 [R + 1]
    value: Tensor             # uint8 [R]

    def to(self, device) -> "FeatureRings":
        return FeatureRings(*(t.to(device) for t in self))


def rings_from_features(features, transform=None, bits: int = 0, value_key: str = "value") -> FeatureRings:
    """The inverse of ``polygons``: GeoJSON-style Polygon and MultiPolygon features (a list of them, or a FeatureCollection) as
    the rings ``ops.scene_burn`` takes after ``.to(device)``, in the order of the features, a polygon's exterior before its
    holes.  ``transform``: None (the coordinates are pixels) or the six numbers (a, b, c, d, e, f) that map pixel (x, y) to
    (a x + b y + c, d x + e y + f), as in ``polygons``: the coordinates go through its inverse.  They are then rounded to the
    nearest 1 / 2^``bits`` pixel (``bits`` 0..8; halves go up), a closing vertex that repeats the first is stripped, and a ring
    is reversed where needed so that, in pixel coordinates with y down, an exterior has a positive shoelace sum (``area2 > 0``)
    and a hole a negative one, which is the orientation of ``ops.scene_rings``.  Every ring of a feature burns
    ``feature["properties"][value_key]``.  A missing value, a value that is no int in 0..255, a geometry that is neither
    Polygon nor MultiPolygon and a singular transform are a ValueError."""
    who = "rings_from_features"
    if isinstance(bits, bool) or not isinstance(bits, int) or not 0 <= bits <= 8:
        raise ValueError(f"{who}: bits must be an int in 0..8, got {bits!r}")
    inverse = None
    if transform is not None:
        try:
            a, b, c, d, e, f = (float(t) for t in transform)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: transform must be None or six numbers (a, b, c, d, e, f), got {transform!r}") from None
        det = a * e - b * d
        if det == 0 or not math.isfinite(det) or not all(math.isfinite(t) for t in (c, f)):
            raise ValueError(f"{who}: the transform {tuple(transform)!r} is singular: it has no inverse")
        inverse = (e / det, -b / det, -d / det, a / det)
    if isinstance(features, dict) and "features" in features:
        features = features["features"]
    scale = 1 << bits
    vertices, offsets, values = [], [0], []
    for k, feature in enumerate(features):
        properties = feature.get("properties") or {}
        if value_key not in properties:
            raise ValueError(f"{who}: feature {k} has no property {value_key!r}")
        v = properties[value_key]
        byte_check(f"{who}: feature {k}", value_key, v)
        geometry = feature.get("geometry") or {}
        kind = geometry.get("type")
        if kind not in ("Polygon", "MultiPolygon"):
            raise ValueError(f"{who}: feature {k}: a Polygon or MultiPolygon geometry is expected, got {kind!r}")
        for polygon in [geometry["coordinates"]] if kind == "Polygon" else geometry["coordinates"]:
            for i, ring in enumerate(polygon):
                points = []
                for X, Y, *_ in ring:
                    if inverse is not None:
                        X, Y = inverse[0] * (X - c) + inverse[1] * (Y - f), inverse[2] * (X - c) + inverse[3] * (Y - f)
                    points.append((math.floor(X * scale + 0.5), math.floor(Y * scale + 0.5)))
                if len(points) > 1 and points[0] == points[-1]:
                    points.pop()
                area2 = sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(points, points[1:] + points[:1]))
                if (area2 < 0) if i == 0 else (area2 > 0):      # an exterior comes first, the holes follow
                    points.reverse()
                vertices += points
                offsets.append(len(vertices))
                values.append(v)
    return FeatureRings(torch.tensor(vertices, dtype=torch.int32).reshape(-1, 2), torch.tensor(offsets, dtype=torch.int32),
                        torch.tensor(values, dtype=torch.uint8))
