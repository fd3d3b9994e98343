"""Host side of whole-scene inference: where the tiles of a scene lie and what window weights them.  The device side is
``gdlhip.ops.scene_cut`` / ``scene_blend`` / ``scene_blend_lowres`` / ``scene_finish`` (include/gdlhip_scene.h); the user-facing
class is ``geo_deep_learning.tools.scene_inference.SceneInference``."""

from __future__ import annotations

import math

import torch
from torch import Tensor


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
