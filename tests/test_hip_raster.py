"""GPU tests of the raster preparation: ``ops.raster_warp`` and ``ops.raster_stats`` (include/gdlhip_raster.h) and the utilities of
``geo_deep_learning.utils.rasters`` over them.

The yardstick of the warp is the float64 restatement of tests/_raster_oracle.py (which tests/test_raster_host.py holds against
Pillow and against results worked out by hand), computed once per case and shared by the dtypes.  Shapes: the warp's workgroup
is 64 x 4 destination pixels, so the destinations below have widths on both sides of 64 and heights that are no multiple of 4,
and reach past every edge of the source; the statistics pass walks 256 x 8 samples per workgroup turn, so 5 x 7 is less than one
workgroup and 61 x 67 is two workgroups and a ragged tail."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
import _raster_oracle as ro  # noqa: E402
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402
from geo_deep_learning.utils import rasters  # noqa: E402

DEV = "cuda"
DTYPES = {"uint8": (np.uint8, torch.uint8), "uint16": (np.uint16, torch.uint16), "int16": (np.int16, torch.int16),
          "float32": (np.float32, torch.float32)}
FILL = 100      # a destination nodata every dtype holds and no exact case produces by chance in a nodata place


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy()


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------ 1. exact warp
# name: (method, source (H, W), (sx, ox, Wd), (sy, oy, Hd)).  Scales in 1, 1/2, 2; offsets multiples of 1/8 (bilinear) and 1/4 (cubic;
# 1/2 at scale 2, where the argument of the kernel is halved once more).  Every destination starts left of and above the source
# and ends right of and below it: pixels wholly outside, pixels whose taps are cut by an edge, and pixels inside.
EXACT = {"bilinear-1": ("bilinear", (19, 23), (1.0, -3.375, 70), (1.0, -2.125, 26)),
         "bilinear-half": ("bilinear", (9, 11), (0.5, -1.625, 67), (0.5, -0.875, 25)),
         "bilinear-2": ("bilinear", (19, 23), (2.0, -4.25, 15), (2.0, -5.125, 14)),
         "bilinear-2-half": ("bilinear", (19, 23), (2.0, -1.875, 13), (0.5, -1.375, 45)),
         "cubic-1": ("cubic", (19, 23), (1.0, -3.25, 70), (1.0, -2.75, 26)),
         "cubic-half": ("cubic", (9, 11), (0.5, -1.75, 67), (0.5, -1.25, 25)),
         "cubic-2": ("cubic", (19, 23), (2.0, -4.0, 15), (2.0, -6.0, 14)),
         "cubic-1-2": ("cubic", (19, 23), (1.0, 0.25, 65), (2.0, -3.5, 13))}


def _exact_source(shape) -> np.ndarray:
    return np.random.default_rng([3, *shape]).integers(0, 64, (2, *shape))      # int64: cast per dtype


@functools.lru_cache(maxsize=None)
def _exact_oracle(name: str, nodata):
    """(source, per band the oracle's sums) of a case, after the assertion that makes the comparison exact: every weight is a
    multiple of 2^-10, so that every product and partial sum is a small multiple of 2^-20 and exact in float64 in any order, and
    every numerator and denominator is a float32."""
    method, shape, (sx, ox, Wd), (sy, oy, Hd) = EXACT[name]
    src = _exact_source(shape)
    if nodata is not None:
        assert (src == nodata).any()
    for n_dst, n_src, s, o in ((Wd, shape[1], sx, ox), (Hd, shape[0], sy, oy)):
        w, _ = ro.axis_taps(n_dst, n_src, s, o, method)
        assert np.array_equal(w * 1024, np.round(w * 1024)), "a weight is no multiple of 2^-10"
    sums = [ro.warp_band(src[c].astype(np.float64), Hd, Wd, sx, ox, sy, oy, method, nodata) for c in range(2)]
    for s in sums:
        assert np.array_equal(s.num.astype(np.float32).astype(np.float64), s.num), "a numerator is no float32"
        assert np.array_equal(s.den.astype(np.float32).astype(np.float64), s.den), "a denominator is no float32"
        assert s.valid.any() and not s.valid.all() and (s.taps == 0).any()
    return src, sums


@pytest.mark.parametrize("nodata", [None, 7], ids=["all-valid", "nodata-7"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(EXACT))
def test_warp_is_exact_where_the_sums_are(name, dtype, nodata):
    method, shape, (sx, ox, Wd), (sy, oy, Hd) = EXACT[name]
    src, sums = _exact_oracle(name, nodata)
    npd, tdt = DTYPES[dtype]
    dev = _dev(src.astype(npd))
    want_valid = np.stack([s.valid for s in sums]).astype(np.uint8)
    with np.errstate(divide="ignore", invalid="ignore"):
        quotient = np.stack([s.num.astype(np.float32) / s.den.astype(np.float32) for s in sums])
    want_f32 = np.where(want_valid > 0, quotient, np.float32(FILL)).astype(np.float32)
    got, valid = ops.raster_warp(dev, (Hd, Wd), sx, ox, sy, oy, method, nodata=nodata, dst_nodata=FILL, out_dtype=torch.float32,
                                 return_valid=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, Hd, Wd) and valid.dtype == torch.uint8
    assert np.array_equal(_np(valid), want_valid)
    assert np.array_equal(_bits(_np(got)), _bits(want_f32)), "float32(num) / float32(den), bit for bit"
    alone = ops.raster_warp(dev, (Hd, Wd), sx, ox, sy, oy, method, nodata=nodata, dst_nodata=FILL, out_dtype=torch.float32)
    assert torch.equal(alone, got), "the call without the plane"
    if dtype != "float32":
        want, want_v, _ = ro.warp(src.astype(npd), (Hd, Wd), sx, ox, sy, oy, method, nodata=nodata, dst_nodata=FILL)
        got, valid = ops.raster_warp(dev, (Hd, Wd), sx, ox, sy, oy, method, nodata=nodata, dst_nodata=FILL, return_valid=True)
        assert got.dtype == tdt and np.array_equal(_np(got), want) and np.array_equal(_np(valid), want_v)


def test_integer_destination_rounds_half_up_and_clamps():
    """Cubic overshoots: a step from 0 to the top of the range goes below 0 and above the top beside the step."""
    for dtype, (lo, hi) in (("uint8", (0, 255)), ("uint16", (0, 65535)), ("int16", (-32768, 32767))):
        npd, _ = DTYPES[dtype]
        src = np.full((1, 6, 12), lo, dtype=npd)
        src[:, :, 6:] = hi
        args = ((6, 24), 0.5, 0.0, 1.0, 0.0, "cubic")
        want, _, sums = ro.warp(src, *args)
        q = sums[0].num / sums[0].den
        assert q.min() < lo and q.max() > hi and want.min() == lo and want.max() == hi
        assert np.array_equal(_np(ops.raster_warp(_dev(src), *args)), want)
    src = np.array([[[0, 1, 2, 3]]], dtype=np.uint8)      # u = 1, 2, 3: halves, rounded up
    assert _np(ops.raster_warp(_dev(src), (1, 3), 1.0, 0.5, 1.0, 0.0, "bilinear")).tolist() == [[[1, 2, 3]]]


NEAREST = {"0.3": ((0.3, -1.1, 90), (0.3, 0.7, 70)), "2.5": ((2.5, -3.3, 12), (2.5, 1.9, 9)), "1": ((1.0, -2.0, 70), (1.0, -1.0, 21))}


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(NEAREST))
def test_nearest_is_exact_at_any_geometry(name, dtype):
    (sx, ox, Wd), (sy, oy, Hd) = NEAREST[name]
    npd, tdt = DTYPES[dtype]
    src = _exact_source((19, 23)).astype(npd)
    for nodata in (None, [7, None]):
        for out in (None, torch.float32):
            want, want_v, _ = ro.warp(src, (Hd, Wd), sx, ox, sy, oy, "nearest", nodata=nodata, dst_nodata=FILL,
                                      out_dtype=None if out is None else np.float32)
            got, valid = ops.raster_warp(_dev(src), (Hd, Wd), sx, ox, sy, oy, "nearest", nodata=nodata, dst_nodata=FILL, out_dtype=out,
                                         return_valid=True)
            assert got.dtype == (tdt if out is None else torch.float32)
            assert np.array_equal(_np(got), want) and np.array_equal(_np(valid), want_v) and 0 < want_v.sum() < want_v.size


# ------------------------------------------------------------------ 2. general geometry
GENERAL = {"0.73x1.37": ((0.73, -2.31, 80), (1.37, -3.17, 37)), "2.5x3.0": ((2.5, -4.71, 25), (3.0, 1.23, 15))}
TIE_BAND = 2.0**-20


def _general_source(dtype: str) -> np.ndarray:
    rng = np.random.default_rng([17, len(dtype)])
    if dtype == "float32":
        src = (rng.standard_normal((2, 41, 53)) * 100).astype(np.float32)
        src[rng.random(src.shape) < 0.1] = -9999.0
        return src
    info = np.iinfo(DTYPES[dtype][0])
    src = rng.integers(info.min, info.max + 1, (2, 41, 53)).astype(DTYPES[dtype][0])
    src[rng.random(src.shape) < 0.1] = info.max      # the nodata value of the masked runs
    return src


@pytest.mark.parametrize("masked", [False, True], ids=["all-valid", "nodata"])
@pytest.mark.parametrize("method", ["bilinear", "cubic"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(GENERAL))
def test_warp_is_within_the_rounding_bound_of_the_oracle(name, dtype, method, masked):
    """float32 output against the float64 oracle: |out - oracle| <= (T + 16) 2^-23 S per pixel, T the taps and S = sum |w m v| /
    sum w m of the oracle: a rounding per product and per sum and up to four per weight would fit in it.  (The kernel carries its
    sums in float64, so what remains is the two conversions and the division.)  The planes must agree wherever the oracle's share
    of unmasked weight is not within 2^-20 of 0.25; the seeds are chosen so that no pixel is."""
    (sx, ox, Wd), (sy, oy, Hd) = GENERAL[name]
    src = _general_source(dtype)
    nodata = None if not masked else -9999.0 if dtype == "float32" else int(np.iinfo(src.dtype).max)
    sums = [ro.warp_band(src[c], Hd, Wd, sx, ox, sy, oy, method, nodata) for c in range(2)]
    got, valid = ops.raster_warp(_dev(src), (Hd, Wd), sx, ox, sy, oy, method, nodata=nodata, dst_nodata=-1.0, out_dtype=torch.float32,
                                 return_valid=True)
    got, valid = _np(got).astype(np.float64), _np(valid)
    for c, s in enumerate(sums):
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(s.tot > 0, s.den / s.tot, np.inf)
        assert not (np.abs(share - ro.MIN_VALID_WEIGHT) <= TIE_BAND).any(), "a pixel of the case lies in the tie band: take another seed"
        assert np.array_equal(valid[c] > 0, s.valid) and 0 < s.valid.sum() < s.valid.size      # the destination reaches past the source
        ok = s.valid
        err, bound = np.abs(got[c][ok] - s.num[ok] / s.den[ok]), (s.taps[ok] + 16) * 2.0**-23 * s.spread[ok]
        print(f"{name} {dtype} {method} band {c}: worst error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert (err <= bound).all()
        assert (got[c][~ok] == -1.0).all()


# ------------------------------------------------------------------ 3. warp edges
def test_one_pixel_destination_and_one_pixel_source():
    src = _exact_source((19, 23)).astype(np.uint16)
    for method in ("nearest", "bilinear", "cubic"):
        want, want_v, _ = ro.warp(src, (1, 1), 1.0, 4.0, 1.0, 6.0, method)
        got, valid = ops.raster_warp(_dev(src), (1, 1), 1.0, 4.0, 1.0, 6.0, method, return_valid=True)
        assert tuple(got.shape) == (2, 1, 1) and np.array_equal(_np(got), want) and want_v.all() and _np(valid).all()
        one = np.array([[[41]]], dtype=np.uint16)      # every destination pixel inside it is that sample, every other nodata
        want, want_v, _ = ro.warp(one, (5, 7), 0.25, -0.25, 0.25, -0.125, method, dst_nodata=9)
        got, valid = ops.raster_warp(_dev(one), (5, 7), 0.25, -0.25, 0.25, -0.125, method, dst_nodata=9, return_valid=True)
        assert np.array_equal(_np(got), want) and np.array_equal(_np(valid), want_v)
        assert set(want[want_v > 0].tolist()) == {41} and set(want[want_v == 0].tolist()) == {9} and want_v.sum() == 4 * 4


@pytest.mark.parametrize("shape", [(1, 63), (3, 64), (5, 65), (9, 129), (130, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_destinations_that_are_no_multiple_of_the_tile(shape):
    """The workgroup covers 4 rows of 64 columns: the last tile of a row and the last row of tiles are cut."""
    Hd, Wd = shape
    src = _exact_source((19, 23)).astype(np.int16) - 30
    sx, sy = min(23.0 / Wd, 4.0), min(19.0 / Hd, 4.0)
    for method in ("nearest", "bilinear", "cubic"):
        want, want_v, sums = ro.warp(src, (Hd, Wd), sx, 0.0, sy, 0.0, method, nodata=-23, dst_nodata=-77, out_dtype=np.float32)
        got, valid = ops.raster_warp(_dev(src), (Hd, Wd), sx, 0.0, sy, 0.0, method, nodata=-23, dst_nodata=-77, out_dtype=torch.float32,
                                     return_valid=True)
        assert np.array_equal(_np(valid), want_v) and want_v.any()
        if method == "nearest":
            assert np.array_equal(_np(got), want)
            continue
        for c, t in enumerate(sums):      # the bound of test 2
            err = np.abs(_np(got)[c].astype(np.float64) - np.where(t.valid, t.num / np.where(t.valid, t.den, 1.0), -77.0))
            assert (err <= np.where(t.valid, (t.taps + 16) * 2.0**-23 * t.spread, 0.0)).all()


def test_refusals_return_their_status_without_a_launch():
    """The scale checks come before any pointer is looked at: the pointers here lead nowhere."""
    raw = _lib.load()
    buf = (C.c_char * 64)()
    a = C.addressof(buf)
    for kw, message in ((dict(sx=0.0), b"scales must be positive"), (dict(sy=-0.5), b"scales must be positive"),
                        (dict(sx=16.25), b"a scale of at most 16"), (dict(sy=16.25, method=2), b"a scale of at most 16")):
        g = {**dict(sx=1.0, sy=1.0, method=1), **kw}
        assert raw.gdl_raster_warp(a, 1, 1, 4, 4, 4, 4, g["sx"], 0.0, g["sy"], 0.0, g["method"], None, None, 0.0, a, 1, None, a, None) == -1
        assert message in raw.gdl_last_error()
    torch.cuda.synchronize()
    src = _dev(np.zeros((1, 4, 4), dtype=np.uint8))
    for kw in (dict(sx=0.0), dict(sy=-1.0), dict(sx=17.0), dict(sy=16.5, method="cubic")):
        with pytest.raises(ValueError, match="raster_warp: "):
            ops.raster_warp(src, (4, 4), **{**dict(sx=1.0, ox=0.0, sy=1.0, oy=0.0), **kw})
    assert tuple(ops.raster_warp(src, (1, 1), 16.0, 0.0, 16.0, 0.0, "cubic").shape) == (1, 1, 1)      # the cap itself goes
    assert tuple(ops.raster_warp(src, (1, 1), 40.0, 0.0, 40.0, 0.0, "nearest").shape) == (1, 1, 1)      # nearest has no cap


# ------------------------------------------------------------------ 4. statistics
def _sums(tiles, nodata):
    """numpy's int64 (integer tiles) or float64 sums per band over the samples that are not nodata: [(count, sum, sum of squares)]."""
    out = []
    for c in range(tiles[0].shape[0]):
        nd = nodata[c] if isinstance(nodata, (list, tuple)) else nodata
        keep = [t[c][~ro.masked(t[c], nd)] for t in tiles]
        wide = np.float64 if tiles[0].dtype == np.float32 else np.int64
        out.append((sum(k.size for k in keep), sum(k.astype(wide).sum() for k in keep), sum((k.astype(wide) ** 2).sum() for k in keep)))
    return out


def _drained(stats: ops.RasterStats):
    stats.drain()
    return list(zip(stats.count, stats.total, stats.total_sq))


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int16"])
def test_integer_statistics_are_exact(dtype):
    npd, _ = DTYPES[dtype]
    info = np.iinfo(npd)
    rng = np.random.default_rng([23, info.bits])
    draw = lambda *shape: rng.integers(info.min, info.max + 1, shape).astype(npd)      # noqa: E731
    # three calls into one accumulator; a shape smaller than one workgroup, one that is no multiple of it, one with two turns
    tiles = [draw(3, 5, 7), draw(3, 5, 7), draw(3, 5, 7)]
    stats = None
    for t in tiles:
        stats = ops.raster_stats(_dev(t), acc=stats)
    assert _drained(stats) == [tuple(int(v) for v in s) for s in _sums(tiles, None)]
    for shape in ((3, 61, 67), (3, 300, 301), (1, 1500, 1450)):      # the last: more than one turn of all the workgroups
        t = draw(*shape)
        t[rng.random(shape) < 0.2] = info.max
        t[-1][rng.random(shape[1:]) < 0.2] = info.min
        per_band = [int(info.max), None, int(info.min)][-shape[0]:]      # a value each, and a band without
        for nodata in (None, int(info.max), per_band):
            assert _drained(ops.raster_stats(_dev(t), nodata)) == [tuple(int(v) for v in s) for s in _sums([t], nodata)], (shape, nodata)


def test_the_accumulator_is_drained_before_it_could_wrap(monkeypatch):
    """uint16 tiles of all 65535 with the drain threshold lowered: the totals are exact Python integers whatever the drains."""
    t = np.full((2, 40, 50), 65535, dtype=np.uint16)
    monkeypatch.setattr(ops, "RASTER_STATS_DRAIN_PIXELS", 5000)
    stats, drains = ops.RasterStats(), []
    real = stats.drain
    monkeypatch.setattr(stats, "drain", lambda: drains.append(stats.pending) or real())
    for _ in range(7):
        ops.raster_stats(_dev(t), acc=stats)
    assert drains == [4000] * 3 and stats.pending == 2000      # 2000 px per call: drained where a call would reach 5000
    means, stds = stats.finish()
    assert stats.count == [14000, 14000] and stats.total == [14000 * 65535] * 2 and stats.total_sq == [14000 * 65535**2] * 2
    assert means == [65535.0, 65535.0] and stds == [0.0, 0.0]


def test_float_statistics_are_within_rounding_and_reproducible():
    rng = np.random.default_rng(29)
    for shape in ((2, 5, 7), (2, 61, 67), (1, 1500, 1450)):      # the last: more than one turn of all the workgroups
        t = (rng.standard_normal(shape) * 1000 + 300).astype(np.float32)
        t[rng.random(shape) < 0.1] = np.nan
        first, second = (_drained(ops.raster_stats(_dev(t), float("nan"))) for _ in range(2))
        assert first == second, "two runs, different bits"
        for (n, s, q), (wn, ws, wq), band in zip(first, _sums([t], float("nan")), t):
            x = band[~np.isnan(band)].astype(np.float64)
            assert n == wn == x.size and isinstance(s, float)
            assert abs(s - ws) <= n * 2.0**-52 * np.abs(x).sum() and abs(q - wq) <= n * 2.0**-52 * (x * x).sum()
    t = np.array([[[1.5, -2.0, 4.0, -2.0]]], dtype=np.float32)
    assert _drained(ops.raster_stats(_dev(t), -2.0)) == [(2, 5.5, 18.25)]
    stats = ops.raster_stats(_dev(t), -2.0)
    assert _drained(ops.raster_stats(_dev(t), None, stats)) == [(6, 7.0, 44.5)]      # accumulated across calls and drains


# ------------------------------------------------------------------ 5. utilities
def from_origin(west, north, xsize, ysize):
    return (xsize, 0.0, west, 0.0, -ysize, north)


def test_compute_dataset_stats_on_the_references_tiles():
    tiles = [torch.full((1, 4, 4), 5.0), torch.full((1, 4, 4), 15.0, device=DEV)]      # a host and a device tile
    assert rasters.compute_dataset_stats(tiles, nodata=-9999) == ([10.0], [5.0])
    assert rasters.compute_dataset_stats(iter(t.to(torch.uint8) for t in tiles)) == ([10.0], [5.0])
    with pytest.raises(ValueError, match="band 0 has no valid pixel"):
        rasters.compute_dataset_stats([torch.full((1, 4, 4), 5.0)], nodata=5.0)


def test_align_to_grid_on_the_references_pair():
    """The reference's test pair: a 5 x 5 input of tens at 2 units per pixel from (0, 10), aligned to the 5 x 5 grid at 1 unit per
    pixel from (0, 5), which it covers; and the other way round, where the input reaches only the lower left of the grid."""
    coarse, fine = from_origin(0, 10, 2, 2), from_origin(0, 5, 1, 1)
    tens = torch.full((5, 5), 10.0)
    out = rasters.align_to_grid(tens, coarse, fine, (5, 5), "nearest", nodata=-32767)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (5, 5) and (out == 10.0).all()
    ramp = torch.arange(25, dtype=torch.int16).reshape(1, 5, 5)
    out, valid = rasters.align_to_grid(ramp.to(DEV), fine, coarse, (5, 5), "nearest", nodata=-32767, return_valid=True)
    assert tuple(out.shape) == (1, 5, 5) and out.dtype == torch.int16
    # destination rows 0, 1 lie north of the input (v = -4, -2), rows 2..4 read its rows 0, 2, 4; columns 0, 1 read 1, 3 (u = 1, 3, 5, ..)
    n = -32767
    assert out[0].tolist() == [[n] * 5, [n] * 5, [1, 3, n, n, n], [11, 13, n, n, n], [21, 23, n, n, n]]
    assert valid[0].tolist() == [[0] * 5, [0] * 5, [1, 1, 0, 0, 0], [1, 1, 0, 0, 0], [1, 1, 0, 0, 0]]
    for method in ("bilinear", "cubic"):
        out = rasters.align_to_grid(tens, coarse, fine, (5, 5), method, nodata=-32767)
        assert tuple(out.shape) == (5, 5) and (out == 10.0).all()
