"""GPU tests of the raster radiometry: ``ops.raster_hist`` with its quantiles, ``ops.raster_stretch``
(include/gdlhip_raster_tone.h), the utilities of ``geo_deep_learning.utils.rasters`` over them and ``SceneInference(stretch=)``.

Every comparison is exact: the yardstick is the numpy float64 restatement of tests/_tone_oracle.py, which
tests/test_raster_tone_host.py holds against ``np.quantile`` and against results worked out by hand.  Shapes: 5 x 7 is less than
one wave; 61 x 67 is odd, so bands 1 and 2 start off a 16-byte boundary (by 2 and 4 bytes for uint16) and the kernels take
their sample-by-sample head and tail; 263 x 257 = 67,591 samples per band is more than the 65,535 a 16-bit counter of the
histogram's LDS table holds, so a workgroup flushes in between."""

import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
import _tone_oracle as to  # noqa: E402
import oracle  # noqa: E402
from gdlhip import ops  # noqa: E402
from geo_deep_learning.models.encoders.dofa_v2 import DOFAv2  # noqa: E402
from geo_deep_learning.models.segmentation.dofa import DOFASegmentationModel  # noqa: E402
from geo_deep_learning.tools.scene_inference import SceneInference  # noqa: E402
from geo_deep_learning.tools.script_model import SegmentationScriptModel  # noqa: E402
from geo_deep_learning.utils import rasters  # noqa: E402
from oracle import procedural_state_dict, synthetic_batch  # noqa: E402
from oracle.model import RGB_MEAN, RGB_STD  # noqa: E402

DEV = "cuda"
NAN = float("nan")
DTYPES = ["uint8", "uint16", "int16", "float32"]
SHAPES = [(2, 5, 7), (3, 61, 67)]
LO, HI = 0.0, 16.0      # the range of the float32 histograms: with a power-of-two bin count every edge is a float32


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def raster(name: str, shape: tuple) -> np.ndarray:
    """Shared by the tests, which leave it unchanged: random samples with both ends of the type, the value 7 (the nodata of the
    tests) and, for float32, samples on lo, on hi, on interior bin edges, below, above, infinite and NaN."""
    rng = np.random.default_rng(sum(shape) + len(name))
    if name == "float32":
        a = rng.uniform(-2.0, 18.0, shape).astype(np.float32)
        a.reshape(shape[0], -1)[:, :12] = [LO, HI, 0.25, 8.0, 15.75, -0.5, 16.5, np.inf, -np.inf, np.nan, 7.0, np.nan]
    else:
        info = np.iinfo(name)
        a = rng.integers(info.min, int(info.max) + 1, shape).astype(name)
        a[rng.random(shape) < 0.3] = 7
        a.reshape(shape[0], -1)[:, :3] = [info.min, info.max, 7]
    return a


def hist_kw(name: str, bins: int = 64) -> dict:
    return dict(bins=bins, value_range=(LO, HI)) if name == "float32" else {}


def nodata_of(shape: tuple):
    return [7, None, 7][:shape[0]]


# ------------------------------------------------------------------ 1. histograms
@pytest.mark.parametrize("with_nodata", [False, True], ids=["all", "nodata"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("name", DTYPES)
def test_hist_equals_the_oracle(name, shape, with_nodata):
    src, nodata = raster(name, shape), nodata_of(shape) if with_nodata else None
    h = ops.raster_hist(_dev(src), nodata, **hist_kw(name))
    want = to.hist(src, nodata, **hist_kw(name))
    assert np.array_equal(_np(h.acc), want)
    assert np.array_equal(_np(h.counts), want[:, :h.bins]) and np.array_equal(_np(h.total), want[:, :h.bins].sum(1))
    assert np.array_equal(_np(h.under), want[:, h.bins]) and np.array_equal(_np(h.over), want[:, h.bins + 1])
    if with_nodata and name != "float32":
        origin = int(to.LAYOUT[src.dtype][1])
        assert want[0, 7 - origin] == 0 and want[1, 7 - origin] > 0      # band 1 has no nodata: its sevens count


@pytest.mark.parametrize("name", ["uint16", "int16"])
def test_hist_of_more_samples_than_a_counter_holds(name):
    """67,591 samples per band: band 0 constant (one 16-bit half takes every sample of a run), band 1 alternating between two
    neighbouring values, the two halves of one LDS word."""
    src = np.empty((2, 263, 257), dtype=name)
    src[0] = 1000
    src[1].reshape(-1)[:] = 1000 + (np.arange(263 * 257) & 1)
    got = _np(ops.raster_hist(_dev(src)).acc)
    origin = int(to.LAYOUT[src.dtype][1])
    assert got[0, 1000 - origin] == 67591 and got[1, 1000 - origin] == 33796 and got[1, 1001 - origin] == 33795
    assert np.array_equal(got, to.hist(src))


@pytest.mark.parametrize("name", DTYPES)
def test_hist_accumulates_and_repeats_bit_for_bit(name):
    a, b = raster(name, (3, 61, 67)), raster(name, (3, 5, 67))
    nodata = nodata_of(a.shape)
    h = ops.raster_hist(_dev(a), nodata, **hist_kw(name))
    assert ops.raster_hist(_dev(b), nodata, h, **hist_kw(name)) is h
    assert np.array_equal(_np(h.acc), to.hist(np.concatenate([a, b], axis=1), nodata, **hist_kw(name)))
    again = ops.raster_hist(_dev(b), nodata, ops.raster_hist(_dev(a), nodata, **hist_kw(name)), **hist_kw(name))
    assert torch.equal(again.acc, h.acc)


@pytest.mark.parametrize("nodata", [None, NAN, [NAN, 7.0, None]], ids=["none", "nan", "per-band"])
@pytest.mark.parametrize("bins", [1, 7, 65536])
def test_hist_of_float32_edges_and_outliers(bins, nodata):
    src = raster("float32", (3, 61, 67))
    ranges = [(LO, HI), (-8.0, 8.0), (0.25, 15.75)]
    got = _np(ops.raster_hist(_dev(src), nodata, bins=bins, value_range=ranges).acc)
    want = to.hist(src, nodata, bins, ranges)
    assert np.array_equal(got, want)
    assert want[0, bins] >= 2 and want[0, bins + 1] >= 2      # -0.5 and -inf under, 16.5 and +inf over
    assert to.hist(src[:1], None, bins, (LO, HI))[0, bins - 1] >= 1      # the sample on hi is in the last bin


# ------------------------------------------------------------------ 2. quantiles
QS = [0.0, 1 / 64, 0.5, 63 / 64, 1.0]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("name", DTYPES)
def test_quantiles_equal_the_oracle(name, shape):
    src, nodata = raster(name, shape), nodata_of(shape)
    kw = hist_kw(name, 256)
    h = ops.raster_hist(_dev(src), nodata, **kw)
    got = h.quantiles(QS)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (shape[0], len(QS))
    want = to.quantiles(to.hist(src, nodata, **kw), *_edges(src, kw, QS))
    assert np.array_equal(_np(got), want)
    if name == "int16":
        assert want[1, 0] == -32768.0 and want[1, -1] == 32767.0      # the origin is applied
    bounds = h.percentile_bounds(2.0, 98.0)
    assert bounds.is_contiguous() and np.array_equal(_np(bounds), to.quantiles(to.hist(src, nodata, **kw), *_edges(src, kw, [0.02, 0.98])))


def _edges(src, kw, qs):
    bins, origin, step = to.edges(src.dtype, src.shape[0], **kw)
    return bins, qs, origin, step


def test_quantiles_of_a_band_without_a_valid_sample_are_nan():
    src = np.array(raster("uint16", (3, 61, 67)))
    src[1] = 9
    got = _np(ops.raster_hist(_dev(src), [None, 9, None]).quantiles(QS))
    assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2]]).any()
    f = np.full((1, 5, 7), np.nan, dtype=np.float32)
    assert np.isnan(_np(ops.raster_hist(_dev(f), NAN, bins=4, value_range=(LO, HI)).quantiles([0.5]))).all()


# ------------------------------------------------------------------ 3. stretch
def _hand_bounds(name: str, channels: int):
    base = {"uint8": (10, 200), "uint16": (1000, 60000), "int16": (-30000, 30000), "float32": (0.5, 15.25)}[name]
    return [base, (7, 7), (NAN, base[1])][:channels] if channels == 3 else [(7, 7), base]


@pytest.mark.parametrize("out", ["uint8", "float32"])
@pytest.mark.parametrize("shape", SHAPES + [(2, 263, 257)], ids=str)
@pytest.mark.parametrize("name", DTYPES)
def test_stretch_equals_the_oracle(name, shape, out):
    src, nodata = raster(name, shape), nodata_of(shape)
    d = _dev(src)
    out_np, out_t = (np.uint8, torch.uint8) if out == "uint8" else (np.float32, torch.float32)
    out_range, fill = ((1, 255), 0) if out == "uint8" else ((-1.0, 2.5), -9.0)
    own = ops.raster_hist(d, nodata, **hist_kw(name, 256)).percentile_bounds(2.0, 98.0)      # stays on the device
    for bounds, host in ((own, _np(own)), (_hand_bounds(name, shape[0]), _hand_bounds(name, shape[0]))):
        dst, valid = ops.raster_stretch(d, bounds, out_range, nodata, fill, out_t, return_valid=True)
        want, want_valid = to.stretch(src, host, out_range, nodata, fill, out_np)
        assert dst.dtype == out_t and np.array_equal(_np(dst).view(np.uint8), want.view(np.uint8))      # bit for bit, NaN-safe
        assert np.array_equal(_np(valid), want_valid)
        assert torch.equal(ops.raster_stretch(d, bounds, out_range, nodata, fill, out_t), dst)      # without the plane
    assert want_valid[0].min() == 0 and want_valid[1].max() == 1
    if shape[0] == 3:
        assert not want_valid[2].any()      # the band of the NaN bound


def test_stretch_rounds_half_up_and_steps_where_the_bounds_meet():
    src = _dev(np.array([[[0, 1, 2, 3, 4]], [[5, 6, 7, 8, 9]]], dtype=np.uint16))
    assert ops.raster_stretch(src, [(0, 4), (7, 7)], (0, 2)).tolist() == [[[0, 1, 1, 2, 2]], [[0, 0, 0, 2, 2]]]


# ------------------------------------------------------------------ 4. the utilities
@pytest.mark.parametrize("name", ["uint16", "float32"])
def test_stretch_to_uint8_is_the_three_calls(name):
    src, nodata = raster(name, (3, 61, 67)), nodata_of((3, 61, 67))
    d, kw = _dev(src), hist_kw(name, 1024)
    bounds = ops.raster_hist(d, nodata, **kw).percentile_bounds(5.0, 95.0)
    want = ops.raster_stretch(d, bounds, (1, 255), nodata, 0, torch.uint8)
    got, used = rasters.stretch_to_uint8(torch.from_numpy(src), percentiles=(5.0, 95.0), nodata=nodata, return_bounds=True, **kw)
    assert got.dtype == torch.uint8 and torch.equal(got, want) and torch.equal(used, bounds)
    assert torch.equal(rasters.stretch_to_uint8(d, bounds=_np(bounds).tolist(), nodata=nodata), want)
    one = rasters.stretch_to_uint8(d[1], percentiles=(5.0, 95.0), **kw)      # [H, W]
    assert one.dim() == 2 and torch.equal(one, rasters.stretch_to_uint8(d[1:2], percentiles=(5.0, 95.0), **kw)[0])


def test_dataset_percentiles_are_those_of_the_union():
    a, b = raster("int16", (3, 61, 67)), raster("int16", (3, 5, 67))
    nodata = nodata_of(a.shape)
    got = rasters.compute_dataset_percentiles([torch.from_numpy(a), _dev(b)], (2.0, 98.0), nodata)
    union = np.concatenate([a, b], axis=1)
    want = to.quantiles(to.hist(union, nodata), *_edges(union, {}, [0.02, 0.98]))
    assert got == want.tolist()


# ------------------------------------------------------------------ 5. SceneInference(stretch=)
@pytest.fixture(scope="module")
def dofa(golden_dir):
    """The tiny DOFA recipe of tests/test_hip_scene.py and a uint16 scene of 11-bit samples, 1.5 tiles on a side, with a corner of
    zeros (its nodata)."""
    meta = json.loads(str(np.load(golden_dir / "dofa_tiny.npz")["meta"]))
    nc, img = 5, meta["img"]
    ref = oracle.DOFASegmentationModel("dofa_tiny_test", (img, img), num_classes=nc, _encoder_kwargs=meta["tiny"], freeze_layers=["encoder"])
    model = DOFASegmentationModel(DOFAv2(img_size=img, pretrained=False, **meta["tiny"]), (img, img), num_classes=nc, pretrained=False,
                                  freeze_layers=["encoder"])
    model.load_state_dict(procedural_state_dict(ref, meta["seed"]))
    model = model.to(DEV).eval()
    batch = synthetic_batch(2, 3, img, nc, meta["seed"])
    sm = SegmentationScriptModel(model, wavelengths=batch["wavelengths"], device=torch.device(DEV), num_classes=nc,
                                 input_shape=(1, 3, img, img), mean=RGB_MEAN, std=RGB_STD)
    side = img + img // 2 + 1
    scene = np.random.default_rng(meta["seed"]).integers(1, 2048, (3, side, side)).astype(np.uint16)
    scene[:, :img // 3, :img // 2] = 0
    return img, sm, torch.from_numpy(scene)


def test_scene_inference_with_stretch_is_the_stretch_by_hand(dofa):
    img, sm, scene = dofa
    kw = dict(tile=(img, img), overlap=0.5, batch_size=64)
    d = scene.to(DEV)
    for nodata in (None, 0):
        bounds = ops.raster_hist(d, nodata).percentile_bounds(2.0, 98.0)
        u8 = ops.raster_stretch(d, bounds, (0, 255), nodata, 0, torch.uint8)
        plane = None if nodata is None else ops.scene_valid(d, nodata)
        want = SceneInference(sm, **kw).predict(u8, return_probs=True, valid=plane)
        got = SceneInference(sm, stretch=(2, 98), nodata=nodata, **kw).predict(scene, return_probs=True)
        assert torch.equal(got.mask, want.mask) and torch.equal(got.probs, want.probs)
        fixed = SceneInference(sm, stretch=_np(bounds).tolist(), nodata=nodata, **kw).predict(scene)
        assert torch.equal(fixed.mask, want.mask)
        assert torch.equal(SceneInference(sm, stretch=bounds, nodata=nodata, **kw).predict(scene).mask, want.mask)
    plain = SceneInference(sm, **kw).predict(u8, return_probs=True)
    same = SceneInference(sm, stretch=None, **kw).predict(u8, return_probs=True)
    assert torch.equal(same.mask, plain.mask) and torch.equal(same.probs, plain.probs)
