"""Host side of the raster preparation (include/gdlhip_raster.h, ``ops.raster_warp`` / ``ops.raster_stats``,
``geo_deep_learning.utils.rasters``), no GPU: the float64 restatement the GPU tests compare with (tests/_raster_oracle.py) held
against Pillow's antialiased resize and against results worked out by hand, the composition of two geotransforms, the errors and
their messages, the arithmetic of ``RasterStats.finish``, and the binding with the refusals that fire before any launch."""

import ctypes as C
import importlib.util
import math

import numpy as np
import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
import _raster_oracle as ro  # noqa: E402
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402
from geo_deep_learning.utils import rasters  # noqa: E402

NAMES = ["gdl_raster_stats", "gdl_raster_stats_workspace", "gdl_raster_warp", "gdl_raster_warp_workspace"]


# ------------------------------------------------------------------ 1. the oracle against Pillow
# (sx, ox, Wd), (sy, oy, Hd): every box lies inside the 37 x 41 image
PILLOW_GEOMETRIES = {"shift": ((1.0, 3.25, 30), (1.0, 2.5, 28)), "up2": ((0.5, 1.0, 60), (0.5, 0.75, 50)),
                     "coarser": ((2.5, 1.5, 15), (3.0, 0.0, 12)), "up3.3": ((0.3, 20.0, 40), (0.3, 15.0, 50))}


@pytest.mark.parametrize("method", ["bilinear", "cubic"])
@pytest.mark.parametrize("geometry", list(PILLOW_GEOMETRIES))
def test_oracle_agrees_with_pillows_antialiased_resize(geometry, method):
    """``Image.resize(box=)`` on a mode-F image is the same edge-renormalised resampling where the box lies inside the image and
    nothing is masked.  Pillow keeps a float32 image between its two passes: differences of a few float32 ulps of 255 (2.4e-4
    was the worst seen) against 1e-1 and more for a wrong tap or kernel.  Bound: 1e-3 absolute."""
    Image = pytest.importorskip("PIL.Image")
    H, W = 37, 41
    img = np.random.default_rng(11).integers(0, 256, (H, W)).astype(np.float32)
    (sx, ox, Wd), (sy, oy, Hd) = PILLOW_GEOMETRIES[geometry]
    assert ox + Wd * sx <= W and oy + Hd * sy <= H
    resample = {"bilinear": Image.Resampling.BILINEAR, "cubic": Image.Resampling.BICUBIC}[method]
    want = np.asarray(Image.fromarray(img).resize((Wd, Hd), resample=resample, box=(ox, oy, ox + Wd * sx, oy + Hd * sy)))
    s = ro.warp_band(img, Hd, Wd, sx, ox, sy, oy, method)
    assert s.valid.all()
    worst = np.abs(s.num / s.den - want.astype(np.float64)).max()
    print(f"{geometry} {method}: worst |oracle - Pillow| = {worst:.3e}")
    assert worst <= 1e-3


# ------------------------------------------------------------------ 2. the validity rule by hand
def test_centre_sample_masked_gives_nodata():
    src = np.arange(9, dtype=np.uint8).reshape(1, 3, 3)
    for method in ("nearest", "bilinear", "cubic"):
        dst, valid, _ = ro.warp(src, (3, 3), 1.0, 0.0, 1.0, 0.0, method, nodata=4, dst_nodata=200)
        assert dst[0, 1, 1] == 200 and valid[0, 1, 1] == 0
        assert valid.sum() == 8 and dst[0, 0, 0] == 0 and dst[0, 2, 2] == 8      # the unmasked centres keep their own sample's pull


def test_cubic_weight_threshold_just_over_and_just_under():
    """A 4 x 4 source, one destination pixel at (u, v) = (2, 2): per axis the taps 0..3 weigh -0.0625, 0.5625, 0.5625, -0.0625 and
    sample 2 contains the centre.  Unmasked (2, 2) alone weighs 0.31640625; with (2, 0) too, 0.28125 >= 0.25: valid, and the value
    is (0.31640625 * 10 - 0.03515625 * 2) / 0.28125 = 11; with (0, 2) as well, 0.24609375 < 0.25: nodata."""
    nd = -1.0
    src = np.full((1, 4, 4), nd, dtype=np.float32)
    src[0, 2, 2], src[0, 2, 0] = 10.0, 2.0
    geometry = (1.0, 1.5, 1.0, 1.5)
    s = ro.warp_band(src[0], 1, 1, *geometry, "cubic", nd)
    assert s.tot[0, 0] == 1.0 and s.den[0, 0] == 0.28125 and s.num[0, 0] == 3.09375 and s.taps[0, 0] == 16
    dst, valid, _ = ro.warp(src, (1, 1), *geometry, "cubic", nodata=nd, dst_nodata=-5.0)
    assert valid[0, 0, 0] == 1 and dst[0, 0, 0] == 11.0
    src[0, 0, 2] = 2.0
    s = ro.warp_band(src[0], 1, 1, *geometry, "cubic", nd)
    assert s.den[0, 0] == 0.24609375 and not s.valid[0, 0]
    dst, valid, _ = ro.warp(src, (1, 1), *geometry, "cubic", nodata=nd, dst_nodata=-5.0)
    assert valid[0, 0, 0] == 0 and dst[0, 0, 0] == -5.0


def test_pixel_outside_the_source_and_at_its_edge():
    src = np.full((1, 4, 5), 7, dtype=np.int16)
    for method in ("nearest", "bilinear", "cubic"):
        dst, valid, sums = ro.warp(src, (2, 3), 1.0, -10.0, 1.0, 0.0, method, dst_nodata=-1)      # ten columns left of the source
        assert (dst == -1).all() and not valid.any() and (sums is None or (sums[0].taps == 0).all())
        dst, valid, _ = ro.warp(src, (2, 3), 1.0, -1.5, 1.0, 2.5, method, dst_nodata=-1)      # u = -1, 0, 1; v = 3, 4
        assert valid[0].tolist() == [[0, 1, 1], [0, 0, 0]] and dst[0].tolist() == [[-1, 7, 7], [-1, -1, -1]]      # edges renormalise


def test_nan_nodata_means_a_nan_sample():
    src = np.array([[[1.0, np.nan, 3.0]]], dtype=np.float32)
    dst, valid, _ = ro.warp(src, (1, 3), 1.0, 0.0, 1.0, 0.0, "bilinear", nodata=float("nan"), dst_nodata=-9.0)
    assert dst[0, 0].tolist() == [1.0, -9.0, 3.0] and valid[0, 0].tolist() == [1, 0, 1]
    dst, valid, _ = ro.warp(src, (1, 2), 1.0, 0.5, 1.0, 0.0, "bilinear", nodata=float("nan"), dst_nodata=-9.0)      # u = 1, 2
    assert valid[0, 0].tolist() == [0, 1] and dst[0, 0, 1] == 3.0      # at u = 2 the NaN's half of the weight is left out
    dst, valid, _ = ro.warp(src, (1, 2), 1.0, 0.5, 1.0, 0.0, "bilinear", dst_nodata=-9.0)      # without nodata the NaN spreads
    assert valid[0, 0].tolist() == [1, 1] and np.isnan(dst[0, 0]).all()


# ------------------------------------------------------------------ 3. geometry, errors, the path wrappers
def from_origin(west, north, xsize, ysize):
    return (xsize, 0.0, west, 0.0, -ysize, north)


def test_grid_to_grid_composes_the_two_transforms():
    assert rasters.grid_to_grid(from_origin(0, 10, 2, 2), from_origin(0, 5, 1, 1)) == (0.5, 0.0, 0.5, 2.5)      # the reference's pair
    assert rasters.grid_to_grid(from_origin(0, 5, 1, 1), from_origin(0, 10, 2, 2)) == (2.0, 0.0, 2.0, -5.0)
    assert rasters.grid_to_grid(from_origin(100, 50, 0.5, 0.25), from_origin(101, 49, 0.5, 0.25)) == (1.0, 2.0, 1.0, 4.0)

    class Affine(tuple):      # rasterio's has nine entries
        pass
    assert rasters.grid_to_grid(Affine((2, 0, 0, 0, -2, 10, 0, 0, 1)), from_origin(0, 5, 1, 1)) == (0.5, 0.0, 0.5, 2.5)


def test_align_to_grid_errors_fire_before_a_device_is_needed():
    src, a, b = torch.zeros((1, 5, 5)), from_origin(0, 10, 2, 2), from_origin(0, 5, 1, 1)
    with pytest.raises(ValueError, match="Unsupported resampling method: lanczos"):
        rasters.align_to_grid(src, a, b, (5, 5), resample_alg="lanczos", nodata=0)
    for rotated in ((2, 0.1, 0, 0, -2, 10), (2, 0, 0, -0.1, -2, 10)):
        with pytest.raises(ValueError, match="Rotated geotransforms are not supported"):
            rasters.align_to_grid(src, rotated, b, (5, 5), nodata=0)
        with pytest.raises(ValueError, match="Rotated geotransforms are not supported"):
            rasters.align_to_grid(src, a, rotated, (5, 5), nodata=0)
    for flipped in ((2, 0, 0, 0, 2, 0), (-2, 0, 10, 0, -2, 10)):      # south-up, east-to-west
        with pytest.raises(ValueError, match="flipped against each other"):
            rasters.align_to_grid(src, flipped, b, (5, 5), nodata=0)
    with pytest.raises(ValueError, match="dst_nodata is needed"):
        rasters.align_to_grid(src, a, b, (5, 5))
    with pytest.raises(ValueError, match="Unsupported resampling method: invalid"):
        rasters.align_to_reference("ref.tif", "in.tif", "out.tif", resample_alg="invalid")


@pytest.mark.skipif(importlib.util.find_spec("rasterio") is not None, reason="rasterio is installed")
def test_path_wrappers_name_the_array_level_function_without_rasterio():
    with pytest.raises(ImportError, match=r"geo_deep_learning\.utils\.rasters\.align_to_grid"):
        rasters.align_to_reference("ref.tif", "in.tif", "out.tif", "nearest")
    with pytest.raises(ImportError, match=r"geo_deep_learning\.utils\.rasters\.compute_dataset_stats"):
        rasters.compute_dataset_stats_from_list(["tile1.tif"])


# ------------------------------------------------------------------ 4. RasterStats.finish
def test_finish_on_given_integers():
    means, stds = ops.RasterStats.from_sums([32], [16 * 5 + 16 * 15], [16 * 25 + 16 * 225]).finish()      # the reference's known answer
    assert means == [10.0] and stds == [5.0]
    # exact where float64 sums of squares would cancel: 2^30 samples of 65535 and one of 65534
    n = (1 << 30) + 1
    s, q = (1 << 30) * 65535 + 65534, (1 << 30) * 65535**2 + 65534**2
    means, stds = ops.RasterStats.from_sums([n, 2], [s, 3], [q, 5]).finish()
    assert means == [s / n, 1.5] and stds[1] == 0.5
    assert stds[0] == math.sqrt((n - 1) / n**2) and stds[0] > 0      # the variance of one outlier by 1: (n - 1) / n^2
    means, stds = ops.RasterStats.from_sums([4], [10.0], [30.0]).finish()      # float sums: float64 throughout
    assert means == [2.5] and stds == [math.sqrt(30.0 / 4 - 6.25)]
    assert ops.RasterStats.from_sums([3], [3.0], [3.0 - 1e-12]).finish()[1] == [0.0]      # rounding below zero is zero


def test_empty_inputs_are_errors_with_the_references_messages():
    with pytest.raises(ValueError, match="No input tiles provided for statistics."):
        rasters.compute_dataset_stats([])
    with pytest.raises(ValueError, match="No input tiles provided for statistics."):
        rasters.compute_dataset_stats_from_list([])
    with pytest.raises(ValueError, match="band 1 has no valid pixel"):
        ops.RasterStats.from_sums([4, 0], [10, 0], [30, 0]).finish()


# ------------------------------------------------------------------ 5. the binding and the checks without a device
def test_raster_header_is_bound_beside_the_other_sets():
    i, l, d, p = C.c_int, C.c_int64, C.c_double, C.c_void_p
    sig = _lib.RASTER_SIGNATURES
    assert sorted(sig) == NAMES
    assert sig["gdl_raster_warp_workspace"] == (l, [i, i, d, d, i]) and sig["gdl_raster_stats_workspace"] == (l, [i, i, i, i])
    assert sig["gdl_raster_warp"] == (i, [p, i, i, i, i, i, i, d, d, d, d, i, p, p, d, p, i, p, p, p])
    assert sig["gdl_raster_stats"] == (i, [p, i, i, i, i, p, p, p, p, p])
    assert not set(sig) & set(_lib.SIGNATURES) and not set(sig) & _lib.STATUS_FUNCTIONS
    assert {"gdl_raster_warp", "gdl_raster_stats"} <= _lib._CHECKED and "gdl_raster_warp_workspace" not in _lib._CHECKED
    assert (_lib.RASTER_NEAREST, _lib.RASTER_BILINEAR, _lib.RASTER_CUBIC) == (0, 1, 2)
    assert _lib.RASTER_MIN_VALID_WEIGHT == ro.MIN_VALID_WEIGHT == 0.25 and _lib.RASTER_MAX_SCALE == 16
    assert _lib.Header("#define GDL_A 0.25\n#define GDL_B -3\n").constants == {"GDL_A": 0.25, "GDL_B": -3}


def test_raster_functions_refuse_before_any_launch():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    raw, checked = _lib.load(), _lib.checked()
    buf = (C.c_char * 64)()
    a = C.addressof(buf)      # never followed: every call below is refused first

    def warp(kind=1, Cc=1, H=4, W=4, Hd=4, Wd=4, sx=1.0, ox=0.0, sy=1.0, oy=0.0, method=1, dst_kind=1, src=a, dst=a, ws=a):
        return raw.gdl_raster_warp(src, kind, Cc, H, W, Hd, Wd, sx, ox, sy, oy, method, None, None, 0.0, dst, dst_kind, None, ws, None)

    refused = {"the scales must be positive": [dict(sx=0.0), dict(sy=-1.0), dict(sx=float("nan")), dict(sy=float("inf"))],
               "a scale of at most 16": [dict(sx=16.5), dict(sy=17.0, method=2)],
               "Hd * Wd < 2^31": [dict(Hd=65536, Wd=32768), dict(Hd=0)],
               "H * W < 2^31": [dict(H=65536, W=32768), dict(W=0), dict(Cc=0), dict(Cc=65536)],
               "bad sample kind": [dict(kind=4)], "method 3 is none of": [dict(method=3)],
               "the offsets must be finite": [dict(ox=float("inf"))],
               "or float32, got kind 0": [dict(dst_kind=0)], "null pointer": [dict(src=None), dict(dst=None)],
               "ws must be given": [dict(ws=None), dict(ws=a + 4)]}
    for message, cases in refused.items():
        for kw in cases:
            assert warp(**kw) == -1 and message.encode() in raw.gdl_last_error(), (kw, raw.gdl_last_error())
    assert raw.gdl_raster_warp_workspace(4, 4, 0.0, 1.0, 1) == -1 and raw.gdl_raster_warp_workspace(4, 4, 1.0, 16.5, 2) == -1
    assert raw.gdl_raster_warp_workspace(4, 4, 100.0, 0.01, 0) == 0      # nearest takes any scale and no table
    # per axis (taps + 1) float64 and three int32 per entry: bilinear at scale 1 has at most 3 taps, cubic at 2.5 at most 11
    assert raw.gdl_raster_warp_workspace(5, 7, 1.0, 1.0, 1) == (5 + 7) * (4 * 8 + 12)
    assert raw.gdl_raster_warp_workspace(5, 7, 2.5, 1.0, 2) == 7 * (12 * 8 + 12) + 5 * (6 * 8 + 12)
    with pytest.raises(ValueError, match="gdl_raster_warp: the scales must be positive and finite, got sx -2, sy 1"):
        checked.gdl_raster_warp(a, 1, 1, 4, 4, 4, 4, -2.0, 0.0, 1.0, 0.0, 1, None, None, 0.0, a, 1, None, a, None)

    def stats(kind=1, Cc=1, H=4, W=4, src=a, acc=a, ws=a):
        return raw.gdl_raster_stats(src, kind, Cc, H, W, None, None, acc, ws, None)

    for message, kw in (("H * W < 2^31", dict(H=65536, W=32768)), ("bad sample kind", dict(kind=-1)), ("null pointer", dict(acc=None)),
                        ("float32 needs ws", dict(kind=3, ws=None)), ("acc to 8 bytes", dict(acc=a + 4))):
        assert stats(**kw) == -1 and message.encode() in raw.gdl_last_error(), (kw, raw.gdl_last_error())
    assert raw.gdl_raster_stats_workspace(1, 3, 5, 7) == 0 and raw.gdl_raster_stats_workspace(3, 3, 5, 7) == 3 * _lib.RASTER_STATS_BLOCKS * 24
    assert raw.gdl_raster_stats_workspace(3, 3, 65536, 32768) == -1


def test_ops_check_their_arguments_before_a_device_is_needed():
    u16 = torch.zeros((2, 4, 5), dtype=torch.uint16)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.raster_warp(u16, (4, 5), 1.0, 0.0, 1.0, 0.0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.raster_stats(u16)
    for bad in (torch.zeros((4, 5), dtype=torch.uint8), torch.zeros((1, 4, 5), dtype=torch.int32), torch.zeros((1, 0, 5)), u16[:, :, ::2], None):
        with pytest.raises(ValueError, match=r"raster_warp: contiguous non-empty \[C, H, W\]"):
            ops.raster_warp(bad, (4, 5), 1.0, 0.0, 1.0, 0.0)
        with pytest.raises(ValueError, match=r"raster_stats: contiguous non-empty \[C, H, W\]"):
            ops.raster_stats(bad)
    with pytest.raises(ValueError, match="raster_warp: unknown method 'lanczos'"):
        ops.raster_warp(u16, (4, 5), 1.0, 0.0, 1.0, 0.0, "lanczos")
    with pytest.raises(ValueError, match="out_dtype must be the source's"):
        ops.raster_warp(u16, (4, 5), 1.0, 0.0, 1.0, 0.0, out_dtype=torch.uint8)
    for bad in ((4,), (0, 5), (65536, 32768), None):
        with pytest.raises(ValueError, match="raster_warp: dst_shape"):
            ops.raster_warp(u16, bad, 1.0, 0.0, 1.0, 0.0)
    for bad, match in ((-1, "outside 0..65535"), (1.5, "not an integer"), ([1, 2, 3], "3 nodata values for 2 bands"), (float("nan"), "NaN nodata needs a float32")):
        with pytest.raises(ValueError, match=match):
            ops.raster_warp(u16, (4, 5), 1.0, 0.0, 1.0, 0.0, nodata=bad)
        with pytest.raises(ValueError, match=match):
            ops.raster_stats(u16, nodata=bad)
    for bad in (-1, 0.5, 65536, float("nan"), "0"):
        with pytest.raises(ValueError, match="raster_warp: dst_nodata"):
            ops.raster_warp(u16, (4, 5), 1.0, 0.0, 1.0, 0.0, dst_nodata=bad)
    for kw, match in ((dict(sx=0.0), "scales must be positive"), (dict(sy=16.5), "a scale of at most 16")):
        with pytest.raises(ValueError, match="raster_warp: .*" + match):
            ops.raster_warp(u16, (4, 5), **{**dict(sx=1.0, ox=0.0, sy=1.0, oy=0.0), **kw})
    values, present = ops.raster_nodata("op", [None, 7], torch.uint16, 2)
    assert list(values) == [0.0, 7.0] and list(present) == [0, 1]
    assert ops.raster_nodata("op", None, torch.uint16, 2) == (None, None) == ops.raster_nodata("op", [None, None], torch.uint16, 2)
    assert list(ops.raster_nodata("op", 0.1, torch.float32, 1)[0]) == [float(np.float32(0.1))]      # compared as the samples were rounded
    with pytest.raises(ValueError, match="acc must be a RasterStats"):
        ops.raster_stats(u16, acc=torch.zeros(3))
