"""Whole-scene inference: an ortho-image or satellite scene of any H x W in, one label mask (and, on request, the blended class
probabilities) out.  The scene is covered by overlapping tiles (``gdlhip.scene.plan_tiles``); per batch of tiles one kernel cuts
and normalises them (``ops.scene_cut``), the exported model (a ``ScriptModel``) runs, and one kernel adds the window-weighted
class probabilities into a canvas [K+1, H, W] -- straight from the heads' low-resolution maps where the model hands them over
(``ops.scene_blend_lowres``: the [B, K, th, tw] probabilities are never written), otherwise from ``class_probs``
(``ops.scene_blend``).  ``ops.scene_finish`` labels the canvas once at the end.

Test-time augmentation (``tta=``): every tile is fed once per transform of ``gdlhip.scene.tta_codes`` (flips, or all eight
symmetries of the square), the tile list becoming (origin, transform) pairs (``gdlhip.scene.plan_tta``).  The cut writes the
transformed tile and the blend reads the model's answer back through the inverse transform (``ops.scene_cut_d4`` /
``scene_blend_d4`` / ``scene_blend_lowres_d4``): the transform lives in the index arithmetic of the two gathers, nothing is
permuted in memory, and the canvas simply collects G times the weight.

Nodata (``nodata=`` and / or ``valid=``): a validity plane of the raster (``ops.scene_valid`` from one nodata value per band, or
the caller's own mask, or both ANDed) decides three things.  The tiles that hold fewer than ``min_valid`` valid pixels are dropped
from the plan before the model sees them (``ops.scene_tile_valid``: one launch and one small copy for the whole plan); an invalid
pixel inside a kept tile reaches the model as the raw value ``fill``, like a position outside the raster (``ops.scene_cut_valid``);
and the mask says ``nodata_label`` where the plane is 0 or no kept tile covers the pixel (``ops.scene_finish_valid``).  The blends
are untouched, and without ``nodata=`` and ``valid=`` so is everything else.

Sieve (``sieve=``): the finished mask is cleaned of speckle on the device before it is returned.  ``ops.scene_sieve`` labels its
connected components and gives every component of fewer than ``sieve`` pixels (the minimum mapping unit) the class of the largest
neighbour that is at least that large; ``nodata_label`` pixels are left alone where a validity plane is in play.  The sieve edits
the map, not the probabilities: ``probs`` are returned as blended.

Polygons (``predict_rings``): the boundaries of the mask's regions as closed rings of lattice points, traced on the device
(``ops.scene_rings``), the step GDAL polygonize takes on the host; ``gdlhip.scene.polygons`` groups them into features with holes.
``predict_rings(simplify=tolerance)`` simplifies them on the device before they leave it (``ops.scene_rings_simplify``):
Douglas-Peucker per arc between the junctions of the boundaries, so that a boundary two regions share stays shared.

Attributes (``predict_features``): beside the rings, what a vector layer says about each polygon -- pixel count, bounding box,
centroid sums and the model's mean and lowest confidence in the region -- reduced on the device from the mask, its component
labels and the canvas (``ops.scene_regions``); neither the probabilities nor the mask have to leave the device for them.

Agreement (``agreement=True`` on ``predict_rings`` / ``predict_features``, or ``rings_agreement``): the rings burned back into a
raster on the device (``ops.scene_burn``, the step GDAL rasterize takes) and compared with the mask: how many pixels the
simplification moved to another class, how many lie where simplified arcs crossed, and the per-class counts behind an IoU.

Stretch (``stretch=``): a uint16 / int16 / float32 scene is brought into the 8-bit range the model was trained on before it is
cut: every band stretched linearly to the model's ``image_min..image_max`` and clipped, by the raster's own percentiles
(``ops.raster_hist`` and its quantiles) or by given bounds (``ops.raster_stretch``), on the device.  The validity plane is taken
from the original samples first; everything after the upload sees a uint8 raster.

Determinism: the canvas is accumulated by a gather in tile order without atomics, so the mask and the probabilities do not
depend on ``batch_size`` and are the same bits from run to run.  The reference has no counterpart (its inference stops at the
tile, tools/script_model.py)."""

from __future__ import annotations

from typing import NamedTuple

import torch

from gdlhip import nn as gnn
from gdlhip import ops
from gdlhip import scene as gscene

from .script_model import ScriptModel

_RASTER_DTYPES = (torch.uint8, torch.uint16, torch.int16, torch.float32)


class SceneResult(NamedTuple):
    mask: torch.Tensor                  # uint8 [H, W]
    probs: torch.Tensor | None          # f32 [K, H, W], None unless asked for


class SceneVectors(NamedTuple):
    mask: torch.Tensor                  # uint8 [H, W], what ``predict`` returns
    rings: ops.SceneRings               # the rings of its regions, on the device


class SceneFeatures(NamedTuple):
    mask: torch.Tensor                  # uint8 [H, W], what ``predict`` returns
    rings: ops.SceneRings               # the rings of its regions, on the device
    regions: ops.SceneRegions           # the attributes of its regions, on the device


class SceneVectorsAgreement(NamedTuple):
    mask: torch.Tensor                  # as in SceneVectors
    rings: ops.SceneRings
    agreement: dict                     # ``rings_agreement(mask, rings, num_classes)``


class SceneFeaturesAgreement(NamedTuple):
    mask: torch.Tensor                  # as in SceneFeatures
    rings: ops.SceneRings
    regions: ops.SceneRegions
    agreement: dict                     # ``rings_agreement(mask, rings, num_classes)``


def rings_agreement(mask: torch.Tensor, rings, num_classes: int) -> dict:
    """How well ``rings`` (a ``SceneRings`` or what ``ops.scene_burn`` takes, on the mask's device) describe the uint8 [H, W]
    ``mask``: the rings are burned into a raster of the mask's size (background 0, conflict 255) and compared with it.
    ``differ``: the pixels where the two are not equal; ``conflicts``: the pixels the rings cover twice or inside out (crossed
    arcs of a simplification); ``iou_counts``: int64 [3, num_classes] on the device, per class the pixels both have, the burn
    has and the mask has (``ops.iou_counts`` of the burn against the mask; values of ``num_classes`` and above, the conflict
    value among them, count for no class).  Rings of every region of a mask, unsimplified, give ``differ == 0`` wherever the
    mask is not 0 outside the rings (classes that ``values=`` left out, ``nodata_label`` pixels)."""
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= 64:
        raise ValueError(f"rings_agreement: num_classes must be an int in 1..64 (ops.iou_counts), got {num_classes!r}")
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.dim() != 2 or not mask.is_contiguous():
        raise ValueError("rings_agreement: a contiguous uint8 [H, W] mask is expected")
    burn = ops.scene_burn(rings, (int(mask.shape[0]), int(mask.shape[1])), reference=mask)
    counts = ops.iou_counts(burn.mask.long().reshape(1, -1), mask.long().reshape(1, -1), num_classes)[0]
    return {"differ": burn.differ, "conflicts": burn.conflicts, "iou_counts": counts}


class SceneInference:
    """``SceneInference(script_model, tile=(512, 512), overlap=0.5).predict(raster)``.

    ``script_model``: a ``ScriptModel`` / ``SegmentationScriptModel``; its input range, mean, std, bf16 flag and wavelengths apply.
    ``tile``: the model's input size.  ``overlap`` (a fraction of the tile, 0 <= overlap < 1) or ``stride`` = (sy, sx) sets the
    grid: origins 0, s, 2s, ... along an axis and a last one clamped to ``L - tile``; a scene smaller than the tile is one tile
    at the origin, padded with the raw value ``fill``.  ``window``: ``"hann"`` (strictly positive, the default) or ``"flat"``.
    ``lowres=False`` takes the ``class_probs`` + ``scene_blend`` route even where the model returns its heads' maps.
    ``tta``: ``None`` (no augmentation: the calls and the bits of before), ``"flips"`` (identity and the three flips), ``"d4"`` (all
    eight symmetries; a square tile) or a sequence of distinct codes in 0..7 (``gdlhip.scene``: 1 = flip x, 2 = flip y, 4 =
    transpose); the probabilities of a tile's transforms are averaged with the window.  ``batch_size`` then counts
    (tile, transform) pairs.
    ``nodata``: ``None`` (every sample is data), one number or one per band; a NaN means "a NaN sample" (float32 rasters).
    ``nodata_rule``: ``"all"`` (a pixel is invalid when every band is nodata) or ``"any"``.  ``nodata_label``: the mask value, 0..255,
    of an invalid or uncovered pixel.  ``min_valid``: a tile with fewer valid pixels than this is not fed to the model.  They act
    only where ``nodata`` is set or ``predict`` / ``canvas`` / ``tile_plan`` get a ``valid=`` plane (uint8 / bool [H, W], nonzero =
    valid: an alpha band, a mask from elsewhere), which is ANDed with the plane of ``nodata``.
    ``sieve``: ``None`` (the mask as labelled: the calls and the bits of before) or the minimum mapping unit in pixels: a connected
    region of one class with fewer pixels takes the class of its largest neighbouring region of at least that many (equally large:
    the lower class), a region with no such neighbour stays (``ops.scene_sieve``).  ``sieve_connectivity``: 4 or 8, for the regions
    and for what counts as a neighbour.  ``sieve_iterations``: how often the labelling and the sieve are repeated.  With a validity
    plane the ``nodata_label`` pixels are no region: they are never changed and no pixel takes their label.  ``probs`` are the
    blended probabilities either way, so where the sieve changed a pixel their arg-max is no longer the mask.
    ``predict_rings`` goes on from the mask to the polygon rings of its regions, and with ``simplify=`` to their Douglas-Peucker
    simplification per shared arc (``ops.scene_rings`` / ``ops.scene_rings_simplify``).
    ``stretch``: ``None`` (the raster as given: the calls and the bits of before), a ``(lo_pct, hi_pct)`` pair of percentiles of the
    uploaded raster itself, or fixed per-band bounds, C ``(lo, hi)`` pairs or a float64 [C, 2] tensor (those of the training set,
    say).  The raster is replaced by its uint8 stretch from those bounds to the model's ``image_min..image_max`` (both must lie
    in 0..255), a sample equal to its band's ``nodata`` becoming ``fill``, which must then be a byte.  The percentiles leave out
    the samples equal to ``nodata`` and nothing more: a ``valid=`` plane does not enter them.  A float32 raster takes fixed
    bounds only (its histogram would need a value range)."""

    def __init__(self, script_model: ScriptModel, tile: tuple[int, int] = (512, 512), overlap: float = 0.5,
                 stride: tuple[int, int] | None = None, window: str = "hann", batch_size: int = 64, threshold: float = 0.5,
                 fill: int = 0, *, lowres: bool = True, tta=None, nodata=None, nodata_rule: str = "all", nodata_label: int = 255,
                 min_valid: int = 1, sieve: int | None = None, sieve_connectivity: int = 4, sieve_iterations: int = 1,
                 stretch=None) -> None:
        if not isinstance(script_model, ScriptModel):
            raise TypeError(f"SceneInference: a ScriptModel is expected, got {type(script_model).__name__}")
        self.model = script_model
        self.tile = (int(tile[0]), int(tile[1]))
        if stride is None:
            if not 0.0 <= overlap < 1.0:
                raise ValueError(f"SceneInference: overlap {overlap} must be in [0, 1)")
            stride = tuple(max(1, round(t * (1.0 - overlap))) for t in self.tile)
        self.stride = (int(stride[0]), int(stride[1]))
        gscene.axis_origins(self.tile[0], self.tile[0], self.stride[0])      # 1 <= stride <= tile, or ValueError
        gscene.axis_origins(self.tile[1], self.tile[1], self.stride[1])
        if batch_size < 1:
            raise ValueError(f"SceneInference: batch_size {batch_size}")
        self.batch_size, self.threshold, self.fill, self.lowres = int(batch_size), float(threshold), int(fill), bool(lowres)
        self.tta = None if tta is None else gscene.tta_codes(tta, self.tile)      # ValueError for what is no set of codes
        if nodata_rule not in ops.NODATA_RULES:
            raise ValueError(f"SceneInference: unknown nodata_rule {nodata_rule!r} ('all' or 'any')")
        ops.byte_check("SceneInference", "nodata_label", nodata_label)
        if isinstance(min_valid, bool) or not isinstance(min_valid, int) or min_valid < 1:
            raise ValueError(f"SceneInference: min_valid must be a pixel count of at least 1, got {min_valid!r}")
        if nodata is not None:      # numbers, one or one per band; whether the raster's type can hold them is checked with the raster
            ops.scene_nodata_values(nodata, torch.float32, script_model.mean.numel(), "SceneInference")
        self.nodata, self.nodata_rule, self.nodata_label, self.min_valid = nodata, nodata_rule, nodata_label, min_valid
        if sieve is not None and (isinstance(sieve, bool) or not isinstance(sieve, int) or sieve < 1):
            raise ValueError(f"SceneInference: sieve must be None or a pixel count of at least 1, got {sieve!r}")
        if isinstance(sieve_connectivity, bool) or sieve_connectivity not in (4, 8):
            raise ValueError(f"SceneInference: sieve_connectivity must be 4 or 8, got {sieve_connectivity!r}")
        if isinstance(sieve_iterations, bool) or not isinstance(sieve_iterations, int) or sieve_iterations < 1:
            raise ValueError(f"SceneInference: sieve_iterations must be an int of at least 1, got {sieve_iterations!r}")
        self.sieve, self.sieve_connectivity, self.sieve_iterations = sieve, sieve_connectivity, sieve_iterations
        self.stretch = None if stretch is None else self._stretch_spec(stretch)
        dev = script_model.device
        self.wy, self.wx = gscene.window(self.tile[0], window).to(dev), gscene.window(self.tile[1], window).to(dev)

    def _stretch_spec(self, stretch):
        """("percentiles", (lo, hi)) or ("bounds", C pairs or a float64 [C, 2] tensor), checked against the model and ``fill``."""
        m, bands = self.model, self.model.mean.numel()
        if not all(isinstance(v, (int, float)) and 0 <= v <= 255 for v in (m.image_min, m.image_max)):
            raise ValueError(f"SceneInference: stretch needs the model's image_min / image_max in 0..255, got {m.image_min!r}, {m.image_max!r}")
        if not ops.is_byte(self.fill):
            raise ValueError(f"SceneInference: with stretch the cut reads a uint8 raster, so fill must be an int in 0..255, got {self.fill!r}")
        if isinstance(stretch, torch.Tensor):
            if stretch.dtype != torch.float64 or tuple(stretch.shape) != (bands, 2):
                raise ValueError(f"SceneInference: stretch bounds must be float64 [{bands}, 2], got {stretch.dtype} {tuple(stretch.shape)}")
            return "bounds", stretch.contiguous()
        number = lambda v: not isinstance(v, bool) and isinstance(v, (int, float))      # noqa: E731
        if isinstance(stretch, (list, tuple)) and len(stretch) == 2 and all(number(v) for v in stretch):
            if not 0.0 <= stretch[0] <= stretch[1] <= 100.0:
                raise ValueError(f"SceneInference: stretch percentiles must be 0 <= lo <= hi <= 100, got {stretch!r}")
            return "percentiles", (float(stretch[0]), float(stretch[1]))
        if isinstance(stretch, (list, tuple)) and len(stretch) == bands and all(
                isinstance(p, (list, tuple)) and len(p) == 2 and all(number(v) for v in p) for p in stretch):
            return "bounds", [(float(lo), float(hi)) for lo, hi in stretch]
        raise ValueError(f"SceneInference: stretch must be None, a (lo_pct, hi_pct) pair, or {bands} (lo, hi) pairs / a float64 "
                         f"[{bands}, 2] tensor, got {stretch!r}")

    def _stretched(self, raster: torch.Tensor) -> torch.Tensor:
        """The uploaded raster as its uint8 stretch to the model's input range (``stretch=``)."""
        m = self.model
        kind, spec = self.stretch
        if kind == "percentiles":
            spec = ops.raster_hist(raster, self.nodata).percentile_bounds(*spec)
        return ops.raster_stretch(raster, spec, (m.image_min, m.image_max), self.nodata, self.fill, torch.uint8)

    def _blend(self, out, origins: torch.Tensor, canvas: torch.Tensor, box: tuple[int, int, int, int],
               xforms: torch.Tensor | None = None) -> None:
        """``xforms``: the batch's transform codes (already checked by ``tta_codes``), None without augmentation."""
        if isinstance(out, gnn.LowresLogits) and self.lowres:
            low = out.low
            if low.dtype == torch.float32 and low.dim() == 4 and 1 <= low.shape[3] <= 16:
                if xforms is None:
                    ops.scene_blend_lowres(low.contiguous(), self.tile, origins, self.wy, self.wx, canvas, box)
                else:
                    ops.scene_blend_lowres_d4(low.contiguous(), self.tile, origins, xforms, self.wy, self.wx, canvas, box, check_codes=False)
                return
        if xforms is None:
            ops.scene_blend(gnn.predict_probs(out), origins, self.wy, self.wx, canvas, box)
        else:
            ops.scene_blend_d4(gnn.predict_probs(out), origins, xforms, self.wy, self.wx, canvas, box, check_codes=False)

    def _upload(self, raster: torch.Tensor, valid: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor | None]:
        """The raster on the device and its validity plane (uint8 [H, W] on the device), None where neither ``nodata`` nor
        ``valid`` is given.  Every argument is checked before anything is uploaded."""
        m = self.model
        if raster.dim() != 3 or raster.dtype not in _RASTER_DTYPES:
            raise ValueError(f"SceneInference: a [C, H, W] uint8/uint16/int16/float32 raster is expected, got {raster.dtype} {tuple(raster.shape)}")
        if raster.shape[0] != m.mean.numel():
            raise ValueError(f"SceneInference: the raster has {raster.shape[0]} channels, the model's mean / std have {m.mean.numel()}")
        _, H, W = raster.shape
        if self.nodata is not None:
            ops.scene_nodata_values(self.nodata, raster.dtype, raster.shape[0], "SceneInference")
        if valid is not None and (valid.dtype not in (torch.uint8, torch.bool) or tuple(valid.shape) != (H, W)):
            raise ValueError(f"SceneInference: valid must be a uint8 / bool [H, W] = [{H}, {W}] plane, got {valid.dtype} {tuple(valid.shape)}")
        if self.stretch is not None and self.stretch[0] == "percentiles" and raster.dtype == torch.float32:
            raise ValueError("SceneInference: a float32 raster needs fixed stretch bounds, not percentiles")
        raster = raster.to(m.device).contiguous()      # a host raster is uploaded once
        plane = None if valid is None else valid.to(m.device).contiguous()
        if self.nodata is not None:
            own = ops.scene_valid(raster, self.nodata, self.nodata_rule)
            plane = own if plane is None else ((own != 0) & (plane != 0)).view(torch.uint8)
        if self.stretch is not None:      # after the plane: that is of the original samples
            raster = self._stretched(raster)
        return raster, plane

    def _plan(self, H: int, W: int, plane: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor]:
        """(the origins kept, the valid pixels of every tile of the full plan), both int32 on the host."""
        plan = gscene.plan_tiles(H, W, self.tile, self.stride)
        if plane is None:      # every pixel is data: the part of a tile inside the raster, and nothing is dropped
            area = min(self.tile[0], H) * min(self.tile[1], W)
            return plan, torch.full((plan.shape[0],), area, dtype=torch.int32)
        counts = ops.scene_tile_valid(plane, plan.to(plane.device), self.tile).cpu()
        return plan[counts >= self.min_valid].contiguous(), counts

    def tile_plan(self, raster: torch.Tensor, valid: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """What ``predict`` feeds of ``raster``: (kept_origins int32 [T', 2], counts int32 [T]), both on the host -- the origins
        of ``gdlhip.scene.plan_tiles`` whose tile holds at least ``min_valid`` valid pixels, in plan order, and the number of
        valid pixels of every tile of the full plan.  The model is not run."""
        raster, plane = self._upload(raster, valid)
        return self._plan(int(raster.shape[1]), int(raster.shape[2]), plane)

    def _canvas(self, raster: torch.Tensor, plane: torch.Tensor | None) -> torch.Tensor:
        m = self.model
        _, H, W = raster.shape
        plan, _ = self._plan(H, W, plane)
        K = int(m.num_classes)
        canvas = torch.zeros((K + 1, H, W), device=m.device, dtype=torch.float32)
        if plan.shape[0] == 0:      # no tile holds data: the model is not called
            return canvas
        codes_dev = None
        if self.tta is not None:
            plan, codes = gscene.plan_tta(plan, self.tta)      # (tile, transform) pairs, tile-major: the accumulation order
            codes_dev = codes.to(m.device)
        plan_dev = plan.to(m.device)
        norm = (m.mean, m.std, m.image_min, m.image_max, m.norm_min, m.norm_max, self.fill)
        for i in range(0, plan.shape[0], self.batch_size):
            origins = plan_dev[i:i + self.batch_size]
            xforms = None if codes_dev is None else codes_dev[i:i + self.batch_size]
            if plane is not None:
                tiles = ops.scene_cut_valid(raster, plane, origins, xforms, self.tile, *norm, check_codes=False)
            elif xforms is None:
                tiles = ops.scene_cut(raster, origins, self.tile, *norm)
            else:
                tiles = ops.scene_cut_d4(raster, origins, xforms, self.tile, *norm, check_codes=False)
            out = m.raw_output(tiles)
            with torch.no_grad():
                self._blend(out, origins, canvas, gscene.bounding_box(plan[i:i + self.batch_size], self.tile), xforms)
        return canvas

    def canvas(self, raster: torch.Tensor, valid: torch.Tensor | None = None) -> torch.Tensor:
        """The finished canvas [K+1, H, W] f32 of ``raster``: planes 0..K-1 the weighted probability sums, plane K the weights
        (0 where no tile that was fed covers the pixel)."""
        return self._canvas(*self._upload(raster, valid))

    def _finish(self, canvas: torch.Tensor, plane: torch.Tensor | None, return_probs: bool) -> SceneResult:
        """The canvas labelled and, where configured, sieved."""
        if plane is None:
            mask, probs = ops.scene_finish(canvas, self.threshold, return_probs)
        else:
            mask, probs = ops.scene_finish_valid(canvas, plane, self.nodata_label, self.threshold, return_probs)
        if self.sieve is not None:      # the map alone: probs stay as blended
            mask = ops.scene_sieve(mask, self.sieve, self.sieve_connectivity, None if plane is None else self.nodata_label,
                                   self.sieve_iterations)
        return SceneResult(mask, probs)

    def predict(self, raster: torch.Tensor, return_probs: bool = False, valid: torch.Tensor | None = None) -> SceneResult:
        raster, plane = self._upload(raster, valid)
        return self._finish(self._canvas(raster, plane), plane, return_probs)

    def _num_classes(self) -> int:
        """The classes a mask of this model can hold: two for a one-class (binary) model."""
        return max(2, int(self.model.num_classes))

    def predict_rings(self, raster: torch.Tensor, valid: torch.Tensor | None = None, *, connectivity: int = 4,
                      values=None, simplify: float | None = None, agreement: bool = False) -> SceneVectors | SceneVectorsAgreement:
        """``predict`` as configured (sieve included), then the polygon rings of the mask's regions under ``connectivity``
        (``ops.scene_rings``; ``values``: the classes to keep, None for all).  Where a validity plane is in play -- ``nodata=``
        or ``valid=``, as for the sieve -- the ``nodata_label`` pixels are no region and get no ring.
        ``simplify``: ``None`` (the rings follow every pixel edge: the calls and the bits of before) or a Douglas-Peucker
        tolerance in pixels, 0 .. 2^20: the rings are simplified on the device arc by arc between the junctions of the boundaries
        (``ops.scene_rings_simplify`` with the same mask, ``nodata_label`` rule and ``values``), so neighbouring regions keep one
        common boundary.  ``area2`` stays the area of the pixel ring, and a ring may collapse to fewer than 3 vertices.
        ``gdlhip.scene.polygons(result.rings)`` turns the rings into features.
        ``agreement``: False (the result, the calls and the bits of before) or True: a ``SceneVectorsAgreement``, the same with
        ``rings_agreement(mask, rings, num_classes)`` of the rings it returns beside them."""
        return SceneInference._predict_vectors(self, "predict_rings", False, raster, valid, connectivity, values, simplify, agreement)

    def predict_features(self, raster: torch.Tensor, valid: torch.Tensor | None = None, *, connectivity: int = 4,
                         values=None, simplify: float | None = None, agreement: bool = False) -> SceneFeatures | SceneFeaturesAgreement:
        """``predict_rings`` with the attributes of the regions beside the rings: the mask as ``predict`` gives it (sieve
        included), its components under ``connectivity`` labelled once, and from those labels both the rings
        (``ops.scene_rings``; ``values`` and ``simplify`` as in ``predict_rings``, the same ``nodata_label`` rule) and the
        ``ops.SceneRegions`` of every region (``ops.scene_regions`` with the canvas): pixels, bounding box, coordinate sums and
        the sum and minimum of the pixels' confidence.  ``values`` selects rings only: the regions are those of all classes.
        The confidence of a pixel is the blended probability of the class it finally carries.  After a sieve a dissolved pixel
        counts with the probability of its *new* class, which the model rated low there: a region that absorbed speckle shows a
        lower confidence, which is the point.  The simplification moves vertices, not pixels: the regions are the same with and
        without it.  ``gdlhip.scene.polygons(result.rings, regions=result.regions)`` joins the two into features.
        ``agreement``: as in ``predict_rings``; True gives a ``SceneFeaturesAgreement``."""
        return SceneInference._predict_vectors(self, "predict_features", True, raster, valid, connectivity, values, simplify, agreement)

    def _predict_vectors(self, who: str, with_regions: bool, raster, valid, connectivity, values, simplify, agreement):
        """``predict_rings`` (``with_regions`` False) and ``predict_features`` (True): the mask, its components labelled once, the
        rings from those labels, the regions where asked for, then the simplification and the agreement."""
        if simplify is not None and not ops.simplify_tolerance_ok(simplify):
            raise ValueError(f"SceneInference.{who}: simplify must be None or a finite tolerance in 0..2^20 pixels, got {simplify!r}")
        raster, plane = self._upload(raster, valid)
        canvas = self._canvas(raster, plane)
        mask = self._finish(canvas, plane, False).mask
        ignore = None if plane is None else self.nodata_label      # no validity plane: every pixel is a region's
        labels = ops.scene_components(mask, connectivity, ignore)[0]
        rings = ops.scene_rings(mask, connectivity, ignore, values, labels=labels)
        regions = ops.scene_regions(mask, connectivity, ignore, canvas=canvas, labels=labels) if with_regions else None
        if simplify is not None:
            rings = ops.scene_rings_simplify(rings, mask, simplify, ignore, values)
        found = (mask, rings, regions) if with_regions else (mask, rings)
        if agreement:
            kind = SceneFeaturesAgreement if with_regions else SceneVectorsAgreement
            return kind(*found, rings_agreement(mask, rings, self._num_classes()))
        return (SceneFeatures if with_regions else SceneVectors)(*found)
