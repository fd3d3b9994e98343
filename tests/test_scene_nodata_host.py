"""Host side of nodata for whole-scene inference, no GPU: the binding of include/gdlhip_scene_nodata.h (SCENE_NODATA_SIGNATURES)
beside the four other sets, the argument checks of its entry points, and the nodata-value checks of ``gdlhip.ops`` and
``SceneInference``, which fire before anything touches a device."""

import ctypes as C

import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402
from geo_deep_learning.tools.scene_inference import SceneInference  # noqa: E402
from geo_deep_learning.tools.script_model import ScriptModel  # noqa: E402

NAMES = ["gdl_scene_cut_valid", "gdl_scene_finish_valid", "gdl_scene_tile_valid", "gdl_scene_valid"]


def test_nodata_header_is_bound_beside_the_other_sets():
    i, l, f, d, p = C.c_int, C.c_int64, C.c_float, C.c_double, C.c_void_p
    sig = _lib.SCENE_NODATA_SIGNATURES
    assert sorted(sig) == NAMES
    assert sig["gdl_scene_valid"] == (i, [p, i, i, i, i, p, i, p, p])
    assert sig["gdl_scene_tile_valid"] == (i, [p, i, i, p, i, i, i, p, p])
    assert sig["gdl_scene_cut_valid"] == (i, [p, i, i, i, i, p, p, p, i, i, i, i, p, i, i, d, d, p, p, p])
    assert sig["gdl_scene_finish_valid"] == (i, [p, i, l, f, p, i, p, p, p])
    # the masked cut is gdl_scene_cut_d4 with one more pointer (valid) after W; the masked finish is gdl_scene_finish with
    # (valid, nodata_label) after the threshold
    res, args = _lib.SCENE_TTA_SIGNATURES["gdl_scene_cut_d4"]
    assert sig["gdl_scene_cut_valid"] == (res, args[:5] + [p] + args[5:])
    res, args = _lib.SCENE_SIGNATURES["gdl_scene_finish"]
    assert sig["gdl_scene_finish_valid"] == (res, args[:4] + [p, i] + args[4:])
    for other in (_lib.SIGNATURES, _lib.DEBUG_SIGNATURES, _lib.SCENE_SIGNATURES, _lib.SCENE_TTA_SIGNATURES):
        assert not set(sig) & set(other)
    assert not set(sig) & _lib.STATUS_FUNCTIONS and set(sig) <= _lib._CHECKED
    # the existing sets keep their sizes
    assert len(_lib.SCENE_SIGNATURES) == 4 and len(_lib.SCENE_TTA_SIGNATURES) == 3


def test_nodata_functions_are_exported_and_status_checked():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    raw, checked = _lib.load(), _lib.checked()
    for n, (res, args) in _lib.SCENE_NODATA_SIGNATURES.items():
        assert getattr(raw, n).argtypes == args and getattr(raw, n).restype is res
        assert getattr(checked, n).errcheck is _lib.status_errcheck
    # a bad argument needs no device: the status comes back in load(), an exception in checked()
    null = {
        "gdl_scene_valid": (None, 0, 3, 37, 53, None, 0, None, None),
        "gdl_scene_tile_valid": (None, 37, 53, None, 4, 16, 16, None, None),
        "gdl_scene_cut_valid": (None, 0, 3, 37, 53, None, None, None, 1, 16, 16, 0, None, 0, 255, 0.0, 1.0, None, None, None),
        "gdl_scene_finish_valid": (None, 5, 35, 0.5, None, 255, None, None, None),
    }
    assert sorted(null) == NAMES
    for name, args in null.items():
        assert getattr(raw, name)(*args) == -1
        assert f"{name}: null pointer".encode() in raw.gdl_last_error()
        with pytest.raises(ValueError, match=f"{name}: null pointer"):
            getattr(checked, name)(*args)
    # the other argument checks come before any launch too: the pointers below are never followed
    buf = (C.c_char * 64)()
    a = C.addressof(buf)
    assert raw.gdl_scene_valid(a, 0, 3, 4, 4, a, 2, a, None) == -1 and b"gdl_scene_valid: rule 2" in raw.gdl_last_error()
    assert raw.gdl_scene_valid(a, 4, 3, 4, 4, a, 0, a, None) == -1 and b"gdl_scene_valid: bad sample kind 4" in raw.gdl_last_error()
    assert raw.gdl_scene_tile_valid(a, 4, 4, a, 0, 2, 2, a, None) == -1 and b"gdl_scene_tile_valid: bad sizes" in raw.gdl_last_error()
    assert raw.gdl_scene_tile_valid(a, 4, 4, a, 1, 65536, 65536, a, None) == -1 and b"does not count in an int32" in raw.gdl_last_error()
    for label in (-1, 256):
        assert raw.gdl_scene_finish_valid(a, 1, 4, 0.5, None, label, a, None, None) == -1
        assert f"gdl_scene_finish_valid: nodata_label {label} is not in 0..255".encode() in raw.gdl_last_error()
    assert raw.gdl_scene_finish_valid(a, 0, 4, 0.5, None, 255, a, None, None) == -1 and b"gdl_scene_finish_valid: bad sizes" in raw.gdl_last_error()
    assert raw.gdl_scene_cut_valid(a, 0, 3, 4, 4, a, a, None, 1, 2, 2, 0, a, 7, 7, 0.0, 1.0, a, a, None) == -1
    assert b"gdl_scene_cut_valid: image_max == image_min (7)" in raw.gdl_last_error()


def test_nodata_values_one_or_one_per_band():
    v = ops.scene_nodata_values(0, torch.uint8, 3)
    assert v.dtype == torch.float32 and v.tolist() == [0.0, 0.0, 0.0]
    assert ops.scene_nodata_values([0, 255, 7], torch.uint8, 3).tolist() == [0.0, 255.0, 7.0]
    assert ops.scene_nodata_values(-32767, torch.int16, 2).tolist() == [-32767.0, -32767.0]
    assert ops.scene_nodata_values(65535.0, torch.uint16, 1).tolist() == [65535.0]
    assert ops.scene_nodata_values(torch.tensor([1.0, 2.0]), torch.float32, 2).tolist() == [1.0, 2.0]
    nan = ops.scene_nodata_values(float("nan"), torch.float32, 2)
    assert nan.isnan().all()
    assert ops.scene_nodata_values(0.1, torch.float32, 1).item() == torch.tensor(0.1).item()      # rounded to f32 as the samples were


@pytest.mark.parametrize("nodata,dtype,match", [
    (0.5, torch.uint8, "not an integer"),
    (256, torch.uint8, r"outside 0\.\.255"),
    (-1, torch.uint8, r"outside 0\.\.255"),
    (-1, torch.uint16, r"outside 0\.\.65535"),
    (65536, torch.uint16, r"outside 0\.\.65535"),
    (-32769, torch.int16, r"outside -32768\.\.32767"),
    (32768, torch.int16, r"outside -32768\.\.32767"),
    ([0, 0, 1.25], torch.int16, "not an integer"),
    (float("inf"), torch.int16, "not an integer"),
    (float("nan"), torch.uint8, "NaN nodata needs a float32 raster"),
    (float("nan"), torch.int16, "NaN nodata needs a float32 raster"),
    ([0, 0], torch.uint8, "2 nodata values for 3 bands"),
    ("0", torch.uint8, "one number or one per band"),
    (True, torch.uint8, "one number or one per band"),
    ([], torch.uint8, "one number or one per band"),
], ids=str)
def test_a_nodata_value_that_can_never_match_is_refused(nodata, dtype, match):
    with pytest.raises(ValueError, match="scene_valid: .*" + match):
        ops.scene_nodata_values(nodata, dtype, 3)
    # ops.scene_valid says the same before it asks for a device tensor
    with pytest.raises(ValueError, match="scene_valid: .*" + match):
        ops.scene_valid(torch.zeros((3, 4, 4), dtype=dtype), nodata)


def test_ops_reject_a_bad_rule_and_host_tensors():
    with pytest.raises(ValueError, match="scene_valid: unknown rule 'some'"):
        ops.scene_valid(torch.zeros((3, 4, 4), dtype=torch.uint8), 0, rule="some")
    with pytest.raises(ValueError, match="device tensors"):
        ops.scene_valid(torch.zeros((3, 4, 4), dtype=torch.uint8), 0)
    with pytest.raises(ValueError, match="device tensors"):
        ops.scene_tile_valid(torch.ones((4, 4), dtype=torch.uint8), torch.zeros((1, 2), dtype=torch.int32), (2, 2))
    with pytest.raises(ValueError, match="device tensors"):
        ops.scene_finish_valid(torch.zeros((2, 4, 4)), None)


def _si(**kw) -> SceneInference:
    sm = ScriptModel(torch.nn.Identity(), device=torch.device("cpu"), num_classes=2, input_shape=(1, 3, 16, 16))
    return SceneInference(sm, tile=(16, 16), **kw)


@pytest.mark.parametrize("kw,match", [
    (dict(nodata_rule="some"), "unknown nodata_rule 'some'"),
    (dict(nodata_rule=0), "unknown nodata_rule 0"),
    (dict(nodata_label=256), "nodata_label must be an int in 0..255, got 256"),
    (dict(nodata_label=-1), "nodata_label must be an int in 0..255, got -1"),
    (dict(nodata_label=1.0), "nodata_label must be an int in 0..255"),
    (dict(min_valid=0), "min_valid must be a pixel count of at least 1, got 0"),
    (dict(min_valid=-3), "min_valid must be a pixel count of at least 1"),
    (dict(min_valid=0.5), "min_valid must be a pixel count of at least 1"),
    (dict(nodata="0"), "nodata must be one number or one per band"),
    (dict(nodata=[0, 0]), "2 nodata values for 3 bands"),
], ids=str)
def test_scene_inference_rejects_at_construction(kw, match):
    with pytest.raises(ValueError, match="SceneInference: " + match):
        _si(**kw)


def test_scene_inference_defaults_are_off():
    si = _si()
    assert si.nodata is None and si.nodata_rule == "all" and si.nodata_label == 255 and si.min_valid == 1
    on = _si(nodata=[0, 1, 2], nodata_rule="any", nodata_label=9, min_valid=40)
    assert on.nodata == [0, 1, 2] and on.nodata_rule == "any" and on.nodata_label == 9 and on.min_valid == 40


@pytest.mark.parametrize("nodata,dtype,match", [
    (0.5, torch.uint8, "not an integer"),
    (-32767, torch.uint8, r"outside 0\.\.255"),
    (-32767, torch.uint16, r"outside 0\.\.65535"),
    (40000, torch.int16, r"outside -32768\.\.32767"),
    (float("nan"), torch.int16, "NaN nodata needs a float32 raster"),
], ids=str)
def test_scene_inference_refuses_a_nodata_the_raster_cannot_hold(nodata, dtype, match):
    """The value is fine for some raster (the constructor takes it), not for this one: ``predict``, ``canvas`` and ``tile_plan``
    refuse it before the raster is uploaded."""
    si = _si(nodata=nodata)
    raster = torch.zeros((3, 20, 20), dtype=dtype)
    for call in (si.predict, si.canvas, si.tile_plan):
        with pytest.raises(ValueError, match="SceneInference: .*" + match):
            call(raster)


def test_scene_inference_refuses_a_valid_plane_of_the_wrong_kind():
    si = _si()
    raster = torch.zeros((3, 20, 20), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"SceneInference: valid must be a uint8 / bool \[H, W\] = \[20, 20\]"):
        si.tile_plan(raster, valid=torch.ones((20, 21), dtype=torch.uint8))
    with pytest.raises(ValueError, match="SceneInference: valid must be a uint8 / bool"):
        si.predict(raster, valid=torch.ones((20, 20), dtype=torch.float32))
