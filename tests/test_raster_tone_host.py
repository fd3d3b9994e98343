"""Host side of the raster radiometry (include/gdlhip_raster_tone.h, ``ops.raster_hist`` / ``ops.raster_stretch``, the percentile
and stretch utilities of ``geo_deep_learning.utils.rasters``, ``SceneInference(stretch=)``), no GPU: the numpy restatement the GPU
tests compare with (tests/_tone_oracle.py) held against ``np.quantile(method="lower")`` and against results worked out by hand,
the binding, the refusals that fire before any launch, and the argument checks of the Python layers."""

import ctypes as C

import numpy as np
import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
import _tone_oracle as to  # noqa: E402
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402
from geo_deep_learning.tools import scene_inference as si  # noqa: E402
from geo_deep_learning.utils import rasters  # noqa: E402

NAMES = ["gdl_raster_hist", "gdl_raster_hist_quantiles", "gdl_raster_stretch"]
NAN = float("nan")


# ------------------------------------------------------------------ 1. the oracle against numpy and by hand
@pytest.mark.parametrize("name", ["uint8", "uint16", "int16"])
def test_oracle_quantiles_are_numpys_lower_method(name):
    """q = k / 64 and N = 997 (N - 1 = 996 = 4 * 249): q (N - 1) = k * 15.5625 is an integer for k a multiple of 16 alone, which
    are left to the hand case below, and otherwise at least 1/16 away from one -- asserted, since at an integer rank a rounding
    of q * (N - 1) would decide, in numpy as here."""
    dtype = np.dtype(name)
    info = np.iinfo(dtype)
    rng = np.random.default_rng(3)
    nd, N = int(info.min), 997
    valid = [rng.integers(nd + 1, int(info.max) + 1, N).astype(dtype),      # the whole range, both ends likely near
             (rng.integers(0, 40, N) + nd + 1).astype(dtype)]                # many ties
    valid[0][:2] = info.min + 1, info.max
    src = np.full((2, 29 * 37), nd, dtype=dtype)                             # 997 valid samples per band, the rest nodata
    src[:, :N] = valid
    src = rng.permuted(src, axis=1).reshape(2, 29, 37)
    nodata = [nd, nd]
    ks = [k for k in range(65) if k % 16]
    for k in ks:
        x = k / 64 * 996
        assert abs(x - round(x)) > 1e-9
    qs = [k / 64 for k in ks]
    bins, origin, step = to.edges(dtype, 2)
    got = to.quantiles(to.hist(src, nodata), bins, qs, origin, step)
    want = np.stack([np.quantile(v, qs, method="lower") for v in valid]).astype(np.float64)
    assert np.array_equal(got, want)


def test_oracle_quantiles_by_hand():
    acc = np.zeros((3, 10), dtype=np.int64)
    acc[0, [1, 4, 7]] = [2, 1, 3]      # sorted: 1 1 4 7 7 7; N - 1 = 5
    acc[1, 3] = 5                      # constant
    acc[0, 8], acc[0, 9] = 100, 100    # under and over take no part
    got = to.quantiles(acc, 8, [0.0, 0.2, 0.39, 0.4, 0.5, 0.6, 1.0], [10.0, 0.0, 0.0], [0.5, 1.0, 1.0])
    assert got[0].tolist() == [10.5, 10.5, 10.5, 12.0, 12.0, 13.5, 13.5]      # ranks 0 1 1 2 2 3 5
    assert got[1].tolist() == [3.0] * 7 and np.isnan(got[2]).all()


def test_oracle_float_bins_by_hand():
    src = np.array([[[-1.0, 0.0, 0.25, 0.5, 0.999, 1.0, 1.5, np.inf, -np.inf, np.nan]]], dtype=np.float32)
    assert to.hist(src, None, 4, (0.0, 1.0))[0].tolist() == [1, 1, 1, 2, 2, 2]      # 1.0 == hi goes to the last bin; NaN nowhere
    assert to.hist(src, NAN, 1, (0.0, 1.0))[0].tolist() == [5, 2, 2]
    assert to.hist(src, 0.5, 4, (0.0, 1.0))[0].tolist() == [1, 1, 0, 2, 2, 2]


def test_oracle_stretch_by_hand():
    """Bounds (100, 300) to 1..255: t = (v - 100) / 200, y = 1 + 254 t.  v = 100 -> 1, 300 -> 255, 200 -> 128, below and above clip;
    v = 101: y = 2.27 -> 2; rounding at .5 goes up: bounds (0, 4) to (0, 2) give y = v / 2, so 1 -> 0.5 -> 1 and 3 -> 1.5 -> 2."""
    src = np.array([[[100, 300, 200, 0, 65535, 101, 7]]], dtype=np.uint16)
    dst, valid = to.stretch(src, [(100, 300)], (1, 255), nodata=7, dst_nodata=0)
    assert dst[0, 0].tolist() == [1, 255, 128, 1, 255, 2, 0] and valid[0, 0].tolist() == [1, 1, 1, 1, 1, 1, 0]
    dst, _ = to.stretch(np.array([[[0, 1, 2, 3, 4]]], dtype=np.uint8), [(0, 4)], (0, 2))
    assert dst[0, 0].tolist() == [0, 1, 1, 2, 2]
    dst, valid = to.stretch(src, [(200, 200)], (10, 20))      # hi == lo: a step at lo
    assert dst[0, 0].tolist() == [10, 20, 10, 10, 20, 10, 10] and valid.all()
    dst, valid = to.stretch(src, [(NAN, 300)], (10, 20), dst_nodata=9)      # NaN bounds: the whole band is nodata
    assert (dst == 9).all() and not valid.any()
    f = np.array([[[0.0, 0.5, np.nan, np.inf, -np.inf]]], dtype=np.float32)
    dst, valid = to.stretch(f, [(0.0, 1.0)], (-1.0, 1.0), dst_nodata=-9.0, out_dtype=np.float32)
    assert dst.dtype == np.float32 and dst[0, 0].tolist() == [-1.0, 0.0, -9.0, 1.0, -1.0] and valid[0, 0].tolist() == [1, 1, 0, 1, 1]
    dst, _ = to.stretch(np.array([[[-32768, 0, 32767]]], dtype=np.int16), [(-32768, 32767)], (255, 0))      # an inverted range
    assert dst[0, 0].tolist() == [255, 127, 0]      # 255 - 255 * 32768 / 65535 = 127.498 -> floor(127.998)


# ------------------------------------------------------------------ 2. the binding and the refusals before a launch
def test_tone_header_is_bound_beside_the_other_sets():
    i, d, p = C.c_int, C.c_double, C.c_void_p
    sig = _lib.RASTER_TONE_SIGNATURES
    assert sorted(sig) == NAMES
    assert sig["gdl_raster_hist"] == (i, [p, i, i, i, i, p, p, i, p, p, p, p])
    assert sig["gdl_raster_hist_quantiles"] == (i, [p, i, i, p, i, p, p, p, p])
    assert sig["gdl_raster_stretch"] == (i, [p, i, i, i, i, p, p, p, d, d, d, p, i, p, p])
    assert set(NAMES) <= _lib._CHECKED and not set(NAMES) & _lib.STATUS_FUNCTIONS
    for prefix in _lib.HEADERS:
        if prefix != "RASTER_TONE":
            assert not set(sig) & set(getattr(_lib, f"{prefix}_SIGNATURES".lstrip("_"))), prefix
    assert _lib.HEADERS["RASTER_TONE"] == "gdlhip_raster_tone.h"
    assert (_lib.RASTER_TONE_MAX_BINS, _lib.RASTER_TONE_MAX_Q) == (65536, 64)


def test_tone_functions_refuse_before_any_launch():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    raw, checked = _lib.load(), _lib.checked()
    buf = (C.c_char * 64)()
    a = C.addressof(buf)      # never followed: every call below is refused first
    dbl = lambda *v: (C.c_double * len(v))(*v)      # noqa: E731

    def hist(kind=3, Cc=1, H=4, W=4, bins=16, lo=dbl(0.0), hi=dbl(1.0), src=a, acc=a):
        return raw.gdl_raster_hist(src, kind, Cc, H, W, None, None, bins, lo, hi, acc, None)

    refused = {"takes 1..65536 bins": [dict(bins=0), dict(bins=65537), dict(bins=-1)],
               "must be finite with lo < hi": [dict(lo=dbl(1.0)), dict(lo=dbl(2.0)), dict(hi=dbl(float("inf"))), dict(lo=dbl(NAN)),
                                               dict(lo=dbl(-1.7e308), hi=dbl(1.7e308))],
               "needs lo and hi per band": [dict(lo=None), dict(hi=None)],
               "kind 1 has 65536 bins": [dict(kind=1, bins=256, lo=None, hi=None)],
               "kind 0 has 256 bins": [dict(kind=0, bins=65536, lo=None, hi=None)],
               "lo and hi are for float32 alone": [dict(kind=2, bins=0), dict(kind=1, bins=65536, hi=None)],
               "H * W < 2^31": [dict(H=65536, W=32768), dict(Cc=0), dict(Cc=65536)], "bad sample kind": [dict(kind=4)],
               "null pointer": [dict(src=None), dict(acc=None)], "acc to 8 bytes": [dict(acc=a + 4), dict(src=a + 2)]}
    for message, cases in refused.items():
        for kw in cases:
            assert hist(**kw) == -1 and message.encode() in raw.gdl_last_error(), (kw, raw.gdl_last_error())

    def quant(Cc=1, bins=16, q=dbl(0.5), Q=1, origin=dbl(0.0), step=dbl(1.0), acc=a, out=a):
        return raw.gdl_raster_hist_quantiles(acc, Cc, bins, q, Q, origin, step, out, None)

    refused = {"1..64 quantiles per call": [dict(Q=0), dict(Q=65)], "is not in [0, 1]": [dict(q=dbl(-0.01)), dict(q=dbl(1.01)), dict(q=dbl(NAN))],
               "q[1] = 2 is not in": [dict(q=dbl(0.5, 2.0), Q=2)], "bins 0 must be in": [dict(bins=0)], "bins 65537 must be": [dict(bins=65537)],
               "must be in 1..65535": [dict(Cc=0), dict(Cc=65536)], "must be finite": [dict(origin=dbl(NAN)), dict(step=dbl(float("inf")))],
               "null pointer": [dict(acc=None), dict(out=None), dict(q=None), dict(origin=None), dict(step=None)],
               "8-byte aligned": [dict(acc=a + 4), dict(out=a + 4)]}
    for message, cases in refused.items():
        for kw in cases:
            assert quant(**kw) == -1 and message.encode() in raw.gdl_last_error(), (kw, raw.gdl_last_error())

    def stretch(kind=1, Cc=1, H=4, W=4, bounds=a, out_lo=0.0, out_hi=255.0, dst_nodata=0.0, dst_kind=0, src=a, dst=a):
        return raw.gdl_raster_stretch(src, kind, Cc, H, W, None, None, bounds, out_lo, out_hi, dst_nodata, dst, dst_kind, None, None)

    refused = {"must lie in 0..255 for a uint8": [dict(out_lo=256.0), dict(out_hi=-1.0), dict(out_hi=255.5)],
               "must be finite": [dict(out_lo=NAN), dict(out_hi=float("inf"), dst_kind=3)],
               "is not a value of uint8": [dict(dst_nodata=256.0), dict(dst_nodata=0.5), dict(dst_nodata=NAN), dict(dst_nodata=-1.0)],
               "is beyond float32": [dict(dst_nodata=1e39, dst_kind=3)],
               "uint8 or float32, got kind 1": [dict(dst_kind=1)], "bad sample kind": [dict(kind=-1)], "H * W < 2^31": [dict(H=0)],
               "null pointer": [dict(bounds=None), dict(src=None), dict(dst=None)], "bounds must be 8-byte aligned": [dict(bounds=a + 4)],
               "aligned to their samples": [dict(src=a + 1), dict(dst=a + 2, dst_kind=3)]}
    for message, cases in refused.items():
        for kw in cases:
            assert stretch(**kw) == -1 and message.encode() in raw.gdl_last_error(), (kw, raw.gdl_last_error())
    with pytest.raises(ValueError, match=r"gdl_raster_stretch: out_lo 256 and out_hi 255 must lie in 0\.\.255"):
        checked.gdl_raster_stretch(a, 1, 1, 4, 4, None, None, a, 256.0, 255.0, 0.0, a, 0, None, None)


# ------------------------------------------------------------------ 3. the Python layers without a device
def test_ops_check_their_arguments_before_a_device_is_needed():
    u16, f32 = torch.zeros((2, 4, 5), dtype=torch.uint16), torch.zeros((2, 4, 5))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.raster_hist(u16)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.raster_hist(f32, bins=16, value_range=(0.0, 1.0))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.raster_stretch(u16, [(0, 1), (0, 1)])
    for bad in (torch.zeros((4, 5), dtype=torch.uint8), torch.zeros((1, 4, 5), dtype=torch.int32), u16[:, :, ::2], None):
        with pytest.raises(ValueError, match=r"raster_hist: contiguous non-empty \[C, H, W\]"):
            ops.raster_hist(bad)
        with pytest.raises(ValueError, match=r"raster_stretch: contiguous non-empty \[C, H, W\]"):
            ops.raster_stretch(bad, [(0, 1)])
    for kw in (dict(value_range=(0, 1)), dict(bins=16), dict(bins=65536, value_range=(0, 65535))):
        with pytest.raises(ValueError, match="bins and value_range are for float32 rasters"):
            ops.raster_hist(u16, **kw)
    for bins in (None, 0, 65537, 2.0, True):
        with pytest.raises(ValueError, match="needs bins, an int in 1..65536"):
            ops.raster_hist(f32, bins=bins, value_range=(0, 1))
    for vr in (None, (0,), [(0, 1)] * 3, "01", [(0, 1), (0, "1")]):
        with pytest.raises(ValueError, match="needs value_range, one"):
            ops.raster_hist(f32, bins=4, value_range=vr)
    for vr in ((1, 1), (2, 1), (0, float("inf")), [(0, 1), (NAN, 1)]):
        with pytest.raises(ValueError, match="must be finite with lo < hi"):
            ops.raster_hist(f32, bins=4, value_range=vr)
    with pytest.raises(ValueError, match="acc must be a RasterHist"):
        ops.raster_hist(u16, acc=ops.RasterStats())
    with pytest.raises(ValueError, match="3 nodata values for 2 bands"):
        ops.raster_hist(u16, nodata=[1, 2, 3])
    # an accumulator of another dtype, band count or binning
    held = ops.RasterHist(torch.float32, 2, 16, [(0.0, 1.0), (0.0, 1.0)])
    for src, kw in ((f32, dict(bins=8, value_range=(0, 1))), (f32, dict(bins=16, value_range=(0, 2))), (f32[:1], dict(bins=16, value_range=(0, 1))),
                    (u16, {})):
        with pytest.raises(ValueError, match="the accumulator holds 2 bands of torch.float32 in 16 bins"):
            ops.raster_hist(src, acc=held, **kw)
    with pytest.raises(ValueError, match="no CPU fallback"):      # the same binning goes through to the device check
        ops.raster_hist(f32, acc=held, bins=16, value_range=[(0, 1), (0.0, 1.0)])
    with pytest.raises(ValueError, match="no raster has been added yet"):
        held.quantiles([0.5])
    assert held.bin_edges() == ([0.0, 0.0], [0.0625, 0.0625])
    assert ops.RasterHist(torch.int16, 1, 65536).bin_edges() == ([-32768.0], [1.0])
    held.acc = torch.zeros((2, 18), dtype=torch.int64)      # never read: the arguments are refused first
    for bad in ([], [0.5] * 65, [1.5], [NAN], ["a"], [True]):
        with pytest.raises(ValueError, match="numbers in .0, 1. expected"):
            held.quantiles(bad)
    for bad in ((98, 2), (-1, 50), (0, 101), ("2", 98)):
        with pytest.raises(ValueError, match="0 <= lo_pct <= hi_pct <= 100"):
            held.percentile_bounds(*bad)

    with pytest.raises(ValueError, match="out_dtype must be torch.uint8 or torch.float32"):
        ops.raster_stretch(u16, [(0, 1)] * 2, out_dtype=torch.uint16)
    for bad in ((0,), (0, NAN), (0, float("inf")), "ab", None):
        with pytest.raises(ValueError, match="out_range must be two finite numbers"):
            ops.raster_stretch(u16, [(0, 1)] * 2, out_range=bad)
    for bad in ((0, 256), (-1, 255)):
        with pytest.raises(ValueError, match="must lie in 0..255 for a uint8 destination"):
            ops.raster_stretch(u16, [(0, 1)] * 2, out_range=bad)
    with pytest.raises(ValueError, match="no CPU fallback"):      # float32 takes any finite range
        ops.raster_stretch(u16, [(0, 1)] * 2, out_range=(-1, 256), out_dtype=torch.float32)
    for bad in (256, 0.5, NAN, "0"):
        with pytest.raises(ValueError, match="raster_stretch: dst_nodata"):
            ops.raster_stretch(u16, [(0, 1)] * 2, dst_nodata=bad)
    for bad in ([(0, 1)], [(0, 1), (0,)], None, torch.zeros((2, 2)), torch.zeros((3, 2), dtype=torch.float64), [(0, 1), ("a", 1)]):
        with pytest.raises(ValueError, match="raster_stretch: bounds must be"):
            ops.raster_stretch(u16, bad)


def test_rasters_and_scene_inference_check_their_arguments():
    u16 = torch.zeros((2, 4, 5), dtype=torch.uint16)
    for bad in ((98, 2), (2,), (-1, 5), (5, 101), None):
        with pytest.raises(ValueError, match="percentiles must be"):
            rasters.stretch_to_uint8(u16, percentiles=bad)
        with pytest.raises(ValueError, match="percentiles must be"):
            rasters.compute_dataset_percentiles([u16], percentiles=bad)
        with pytest.raises(ValueError, match="percentiles must be"):
            rasters.compute_dataset_percentiles_from_list(["a.tif"], percentiles=bad)
    with pytest.raises(ValueError, match=r"src must be a \[C, H, W\] or \[H, W\] tensor"):
        rasters.stretch_to_uint8(torch.zeros(5, dtype=torch.uint16))
    with pytest.raises(ValueError, match="are for the raster's own percentiles"):
        rasters.stretch_to_uint8(u16, bounds=[(0, 1), (0, 1)], bins=4)
    with pytest.raises(ValueError, match="No input tiles provided for percentiles."):
        rasters.compute_dataset_percentiles([])
    with pytest.raises(ValueError, match="No input tiles provided for percentiles."):
        rasters.compute_dataset_percentiles_from_list([])

    def model(**kw):
        return si.ScriptModel(torch.nn.Identity(), device=torch.device("cpu"), num_classes=2, input_shape=(1, 3, 16, 16), **kw)

    sm = model()
    assert si.SceneInference(sm, tile=(16, 16)).stretch is None
    assert si.SceneInference(sm, tile=(16, 16), stretch=(2, 98)).stretch == ("percentiles", (2.0, 98.0))
    assert si.SceneInference(sm, tile=(16, 16), stretch=[(0, 1), (2, 3), (4, 5)]).stretch == ("bounds", [(0.0, 1.0), (2.0, 3.0), (4.0, 5.0)])
    assert si.SceneInference(sm, tile=(16, 16), stretch=torch.zeros((3, 2), dtype=torch.float64)).stretch[0] == "bounds"
    for fill in (-1, 256, 4000):
        with pytest.raises(ValueError, match="with stretch the cut reads a uint8 raster, so fill must be an int in 0..255"):
            si.SceneInference(sm, tile=(16, 16), stretch=(2, 98), fill=fill)
    assert si.SceneInference(sm, tile=(16, 16), fill=4000).fill == 4000      # without stretch: as before
    for bad in ((98, 2), (0, 101), [(0, 1)] * 2, torch.zeros((3, 2)), torch.zeros((2, 2), dtype=torch.float64), "p", (2, 98, 99)):
        with pytest.raises(ValueError, match="SceneInference: stretch"):
            si.SceneInference(sm, tile=(16, 16), stretch=bad)
    with pytest.raises(ValueError, match="image_min / image_max in 0..255, got 0, 65535"):
        si.SceneInference(model(image_max=65535), tile=(16, 16), stretch=(2, 98))
    with pytest.raises(ValueError, match="a float32 raster needs fixed stretch bounds"):
        si.SceneInference(sm, tile=(16, 16), stretch=(2, 98)).predict(torch.zeros((3, 16, 16)))
