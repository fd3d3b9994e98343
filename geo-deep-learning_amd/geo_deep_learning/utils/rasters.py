"""Utility functions related to rasters/arrays: the mirror of the reference's ``utils/rasters.py`` on the device.

The work is defined on arrays, geotransforms in and tensors out: ``align_to_grid`` puts a raster on another raster's grid
(``ops.raster_warp``) and ``compute_dataset_stats`` gives the per-band mean and standard deviation of a list of tiles, nodata left
out (``ops.raster_stats``).  ``align_to_reference`` and ``compute_dataset_stats_from_list`` keep the reference's path-level
signatures; they are file I/O around the two and import rasterio when they are called.

Radiometry, which the reference leaves to the caller (its inference takes ``image_min`` / ``image_max`` as given):
``compute_dataset_percentiles`` gives the per-band percentiles of a list of tiles and ``stretch_to_uint8`` brings a uint16 / int16 /
float32 raster into the 8-bit range a model was trained on, by its own percentiles or by given bounds (``ops.raster_hist`` /
``ops.raster_stretch``, include/gdlhip_raster_tone.h).

Departures from the reference, all stated in INTEGRATION.md: no change of CRS (both grids are north-up and in one CRS); a NaN
nodata value means "a NaN sample" (the reference's ``band != nan`` excludes nothing); the resampling and its validity rule are
those of include/gdlhip_raster.h, not GDAL's.
"""

from __future__ import annotations

from collections.abc import Iterable, Sequence

import torch
from torch import Tensor

RESAMPLE_METHODS = ("nearest", "bilinear", "cubic")


def _six(name: str, transform) -> tuple[float, ...]:
    """(a, b, c, d, e, f) of a rasterio ``Affine`` (its first six entries) or of six numbers in that order."""
    t = tuple(float(v) for v in tuple(transform)[:6])
    if len(t) != 6:
        raise ValueError(f"{name} must hold six numbers in Affine order (a, b, c, d, e, f), got {transform!r}")
    return t


def grid_to_grid(src_transform, dst_transform) -> tuple[float, float, float, float]:
    """(sx, ox, sy, oy): destination pixel (y, x) lies at the source pixel coordinates u = (x + 0.5) sx + ox, v = (y + 0.5) sy +
    oy.  Both transforms map (column, row) to world coordinates, X = a col + c and Y = e row + f; a rotated one (b or d nonzero)
    and a flip between the two grids (a scale that is not positive) are a ValueError."""
    sa, sb, sc, sd, se, sf = _six("src_transform", src_transform)
    da, db, dc, dd, de, df = _six("dst_transform", dst_transform)
    if sb or sd or db or dd:
        raise ValueError("Rotated geotransforms are not supported: b and d must be 0 in both transforms.")
    if not sa or not se:
        raise ValueError("src_transform has a pixel size of 0.")
    sx, sy = da / sa, de / se
    if not (sx > 0 and sy > 0):
        raise ValueError(f"The two grids are flipped against each other (scales {sx}, {sy}): flip one of the rasters first.")
    return sx, (dc - sc) / sa, sy, (df - sf) / se


def align_to_grid(src: Tensor, src_transform, dst_transform, dst_shape: tuple[int, int], resample_alg: str = "bilinear",
                  nodata=None, dst_nodata: float | None = None, out_dtype: torch.dtype | None = None, return_valid: bool = False):
    """``src`` ([C, H, W] or [H, W]; uint8/uint16/int16/float32) with the geotransform ``src_transform`` resampled onto the grid
    of ``dst_transform`` and ``dst_shape`` = (height, width): a tensor of that shape on the device (a host tensor is moved to the
    current one), nodata where the input does not reach.  Transforms are six numbers in rasterio ``Affine`` order.  ``nodata``: of
    the source, None, one number or one per band; ``dst_nodata``: what the pixels without data take, by default the source's
    where that is one number.  See ``ops.raster_warp`` for the rest."""
    from gdlhip import ops

    if resample_alg not in RESAMPLE_METHODS:
        msg = f"Unsupported resampling method: {resample_alg}"
        raise ValueError(msg)
    sx, ox, sy, oy = grid_to_grid(src_transform, dst_transform)
    if dst_nodata is None:
        if isinstance(nodata, bool) or not isinstance(nodata, (int, float)):
            raise ValueError("align_to_grid: dst_nodata is needed where nodata is not one number.")
        dst_nodata = nodata
    if not isinstance(src, Tensor) or src.dim() not in (2, 3):
        raise ValueError("align_to_grid: src must be a [C, H, W] or [H, W] tensor.")
    bands = src if src.dim() == 3 else src[None]
    if not bands.is_cuda:
        bands = bands.cuda()
    out = ops.raster_warp(bands.contiguous(), dst_shape, sx, ox, sy, oy, resample_alg, nodata=nodata, dst_nodata=dst_nodata,
                          out_dtype=out_dtype, return_valid=return_valid)
    if src.dim() == 3:
        return out
    return (out[0][0], out[1][0]) if return_valid else out[0]


def compute_dataset_stats(tiles: Iterable[Tensor], nodata=None) -> tuple[list[float], list[float]]:
    """Global per-band (means, stds) over ``tiles``, an iterable of [C, H, W] tensors of one dtype and band count on the device
    or the host (those are moved), the samples equal to their band's ``nodata`` left out (None, one number or one per band).
    Population standard deviation, as the reference's.  Integer tiles are summed exactly."""
    from gdlhip import ops

    stats = None
    for tile in tiles:
        if isinstance(tile, Tensor) and not tile.is_cuda:
            tile = tile.cuda()
        stats = ops.raster_stats(tile.contiguous() if isinstance(tile, Tensor) else tile, nodata, stats)
    if stats is None:
        msg = "No input tiles provided for statistics."
        raise ValueError(msg)
    return stats.finish()


def _percent_pair(who: str, percentiles) -> tuple[float, float]:
    ok = isinstance(percentiles, (list, tuple)) and len(percentiles) == 2 and all(
        not isinstance(p, bool) and isinstance(p, (int, float)) for p in percentiles)
    if not ok or not 0.0 <= percentiles[0] <= percentiles[1] <= 100.0:
        raise ValueError(f"{who}: percentiles must be (lo, hi) with 0 <= lo <= hi <= 100, got {percentiles!r}")
    return float(percentiles[0]), float(percentiles[1])


def _dataset_hist(tiles, nodata, hist_kw):
    from gdlhip import ops

    hist = None
    for tile in tiles:
        if isinstance(tile, Tensor) and not tile.is_cuda:
            tile = tile.cuda()
        hist = ops.raster_hist(tile.contiguous() if isinstance(tile, Tensor) else tile, nodata, hist, **hist_kw)
    if hist is None:
        msg = "No input tiles provided for percentiles."
        raise ValueError(msg)
    return hist


def compute_dataset_percentiles(tiles: Iterable[Tensor], percentiles: tuple[float, float] = (2.0, 98.0), nodata=None,
                                **hist_kw) -> list[list[float]]:
    """Global per-band [lo, hi] percentiles over ``tiles``, an iterable of [C, H, W] tensors of one dtype and band count on the
    device or the host (those are moved), the samples equal to their band's ``nodata`` left out: numpy's
    ``percentile(valid, p, method="lower")`` over all tiles together, from one histogram on the device that every tile adds to.
    Exact for uint8 / uint16 / int16; float32 tiles need ``bins=`` and ``value_range=`` (``ops.raster_hist``) and give the lower
    edge of the percentile's bin.  A band without a valid sample gives NaN."""
    lo, hi = _percent_pair("compute_dataset_percentiles", percentiles)
    return _dataset_hist(tiles, nodata, hist_kw).percentile_bounds(lo, hi).cpu().tolist()


def stretch_to_uint8(src: Tensor, bounds=None, percentiles: tuple[float, float] = (2.0, 98.0), nodata=None,
                     out_range: tuple[float, float] = (1, 255), dst_nodata: int = 0, return_bounds: bool = False, **hist_kw):
    """``src`` ([C, H, W] or [H, W]; uint8/uint16/int16/float32) as uint8, every band stretched linearly from its ``bounds``
    (lo, hi) to ``out_range`` and clipped, nodata samples set to ``dst_nodata`` (``ops.raster_stretch``).  ``bounds``: C (lo, hi)
    pairs or a float64 [C, 2] device tensor, for example the training set's ``compute_dataset_percentiles``; None: the raster's
    own ``percentiles`` with nodata left out -- histogram, quantiles and stretch run on the device one after the other, and
    nothing comes back to the host in between (float32 then needs ``bins=`` and ``value_range=``).  The default ``out_range``
    keeps 0 free for ``dst_nodata``.  With ``return_bounds`` the bounds used come back too (the raster's own: a float64 [C, 2] device tensor)."""
    from gdlhip import ops

    lo, hi = _percent_pair("stretch_to_uint8", percentiles)
    if not isinstance(src, Tensor) or src.dim() not in (2, 3):
        raise ValueError("stretch_to_uint8: src must be a [C, H, W] or [H, W] tensor.")
    bands = src if src.dim() == 3 else src[None]
    if bounds is not None and hist_kw:
        raise ValueError(f"stretch_to_uint8: {sorted(hist_kw)} are for the raster's own percentiles, not for given bounds")
    if not bands.is_cuda:
        bands = bands.cuda()
    bands = bands.contiguous()
    if bounds is None:
        bounds = ops.raster_hist(bands, nodata, **hist_kw).percentile_bounds(lo, hi)
    out = ops.raster_stretch(bands, bounds, out_range, nodata, dst_nodata, torch.uint8)
    out = out if src.dim() == 3 else out[0]
    return (out, bounds) if return_bounds else out


def _rasterio(instead: str):
    try:
        import rasterio
    except ImportError as e:
        msg = f"rasterio is not installed: read the rasters yourself and call geo_deep_learning.utils.rasters.{instead}"
        raise ImportError(msg) from e
    return rasterio


def _torch_dtype(array):
    """A numpy raster as one of the four dtypes the device takes (anything else as float32)."""
    import numpy as np

    return array if array.dtype in (np.uint8, np.uint16, np.int16, np.float32) else array.astype(np.float32)


def align_to_reference(reference_path: str, input_path: str, output_path: str, resample_alg: str = "bilinear",
                       nodata_val: float = -32767) -> None:
    """The reference's ``align_to_reference``: band 1 of ``input_path`` on the grid of ``reference_path``, written to
    ``output_path``.  File I/O around ``align_to_grid``; the two rasters must share their CRS (there is no reprojection)."""
    if resample_alg not in RESAMPLE_METHODS:
        msg = f"Unsupported resampling method: {resample_alg}"
        raise ValueError(msg)
    rasterio = _rasterio("align_to_grid")
    with rasterio.open(reference_path) as ref, rasterio.open(input_path) as src:
        if src.crs != ref.crs:
            msg = f"CRS differ ({src.crs} and {ref.crs}): align_to_reference does not reproject."
            raise ValueError(msg)
        data = _torch_dtype(src.read(1))
        nodata = src.nodata if src.nodata is not None else nodata_val
        out = align_to_grid(torch.from_numpy(data), src.transform, ref.transform, (ref.height, ref.width), resample_alg,
                            nodata=nodata, dst_nodata=nodata)
        profile = src.profile
        profile.update({"crs": ref.crs, "transform": ref.transform, "width": ref.width, "height": ref.height, "nodata": nodata,
                        "dtype": str(data.dtype), "count": 1, "BIGTIFF": "YES", "compress": "lzw"})
        with rasterio.open(output_path, "w", **profile) as dst:
            dst.write(out.cpu().numpy(), 1)


def compute_dataset_stats_from_list(tile_paths: Sequence[str]) -> tuple[list[float], list[float]]:
    """The reference's ``compute_dataset_stats_from_list``: ``compute_dataset_stats`` over the rasters at ``tile_paths``, each
    with the nodata values of its own metadata."""
    if not tile_paths:
        msg = "No input tiles provided for statistics."
        raise ValueError(msg)
    rasterio = _rasterio("compute_dataset_stats")
    from gdlhip import ops

    stats = None
    for path in tile_paths:
        with rasterio.open(path) as src:
            img, nodata = _torch_dtype(src.read()), list(src.nodatavals)
        stats = ops.raster_stats(torch.from_numpy(img).cuda(), nodata, stats)
    return stats.finish()


def compute_dataset_percentiles_from_list(tile_paths: Sequence[str], percentiles: tuple[float, float] = (2.0, 98.0),
                                          **hist_kw) -> list[list[float]]:
    """``compute_dataset_percentiles`` over the rasters at ``tile_paths``, each with the nodata values of its own metadata."""
    lo, hi = _percent_pair("compute_dataset_percentiles_from_list", percentiles)
    if not tile_paths:
        msg = "No input tiles provided for percentiles."
        raise ValueError(msg)
    rasterio = _rasterio("compute_dataset_percentiles")
    from gdlhip import ops

    hist = None
    for path in tile_paths:
        with rasterio.open(path) as src:
            img, nodata = _torch_dtype(src.read()), list(src.nodatavals)
        hist = ops.raster_hist(torch.from_numpy(img).cuda(), nodata, hist, **hist_kw)
    return hist.percentile_bounds(lo, hi).cpu().tolist()
