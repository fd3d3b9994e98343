"""Host side of whole-scene inference, no GPU: the tile grid and the windows of gdlhip/scene.py, and the binding of
include/gdlhip_scene.h (SCENE_SIGNATURES) beside the public set."""

import ctypes as C

import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import _lib  # noqa: E402
from gdlhip import scene as gscene  # noqa: E402

AXES = [(37, 16, 8), (53, 16, 12), (16, 16, 8), (10, 16, 8), (33, 16, 16)]


@pytest.mark.parametrize("L,t,s", AXES)
def test_axis_origins_cover_the_axis(L, t, s):
    o = gscene.axis_origins(L, t, s)
    assert o[0] == 0 and o[-1] == max(L - t, 0)
    assert all(a < b for a, b in zip(o, o[1:])), "strictly ascending: no duplicate"
    covered = set()
    for a in o:
        covered.update(range(a, a + t))
    assert set(range(L)) <= covered
    assert all(b - a <= s for a, b in zip(o, o[1:])), "no step longer than the stride"


@pytest.mark.parametrize("L,t,s", AXES)
def test_plan_tiles_is_the_row_major_product_of_the_axes(L, t, s):
    plan = gscene.plan_tiles(L, 53, (t, 16), (s, 12))
    ys, xs = gscene.axis_origins(L, t, s), gscene.axis_origins(53, 16, 12)
    assert plan.dtype == torch.int32 and tuple(plan.shape) == (len(ys) * len(xs), 2)
    assert plan.tolist() == [[y, x] for y in ys for x in xs]
    assert plan[0].tolist() == [0, 0] and plan[-1].tolist() == [max(L - t, 0), 53 - 16]
    assert gscene.bounding_box(plan, (t, 16)) == (0, max(L, t), 0, 53)


@pytest.mark.parametrize("s", [0, 17, -1])
def test_plan_tiles_rejects_a_stride_outside_1_to_tile(s):
    with pytest.raises(ValueError, match="stride"):
        gscene.axis_origins(37, 16, s)
    with pytest.raises(ValueError, match="stride"):
        gscene.plan_tiles(37, 53, (16, 16), (8, s))


@pytest.mark.parametrize("n", [1, 2, 15, 16, 512])
@pytest.mark.parametrize("kind", ["hann", "flat"])
def test_windows_are_strictly_positive_and_symmetric(kind, n):
    w = gscene.window(n, kind)
    assert w.dtype == torch.float32 and tuple(w.shape) == (n,)
    assert (w > 0).all() and torch.equal(w, w.flip(0))
    if kind == "flat":
        assert torch.equal(w, torch.ones(n))
    else:
        i = torch.arange(n, dtype=torch.float64)
        assert (w.double() - (0.5 - 0.5 * torch.cos(2 * torch.pi * (i + 0.5) / n))).abs().max().item() <= 2.0 ** -24


def test_window_rejects_an_unknown_kind():
    with pytest.raises(ValueError, match="unknown kind"):
        gscene.window(16, "gauss")


def test_scene_header_is_bound_beside_the_public_set():
    i, l, f, d, p = C.c_int, C.c_int64, C.c_float, C.c_double, C.c_void_p
    sig = _lib.SCENE_SIGNATURES
    assert sorted(sig) == ["gdl_scene_blend", "gdl_scene_blend_lowres", "gdl_scene_cut", "gdl_scene_finish"]
    assert sig["gdl_scene_cut"] == (i, [p, i, i, i, i, p, i, i, i, i, p, i, i, d, d, p, p, p])
    assert sig["gdl_scene_blend"] == (i, [p, i, i, i, i, p, p, p, p, i, i, i, i, i, i, p])
    assert sig["gdl_scene_blend_lowres"] == (i, [p, i, i, i, i, i, i, p, p, p, p, i, i, i, i, i, i, p])
    assert sig["gdl_scene_finish"] == (i, [p, i, l, f, p, p, p])
    assert not set(sig) & set(_lib.SIGNATURES) and not set(sig) & _lib.STATUS_FUNCTIONS
    assert not set(sig) & set(_lib.DEBUG_SIGNATURES)


def test_scene_functions_are_exported_and_status_checked():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    raw, checked = _lib.load(), _lib.checked()
    for n, (res, args) in _lib.SCENE_SIGNATURES.items():
        assert getattr(raw, n).argtypes == args and getattr(raw, n).restype is res
        assert getattr(checked, n).errcheck is _lib.status_errcheck
    # a bad argument needs no device: the status comes back in load(), an exception in checked()
    assert raw.gdl_scene_finish(None, 5, 35, 0.5, None, None, None) == -1
    assert b"gdl_scene_finish: null pointer" in raw.gdl_last_error()
    with pytest.raises(ValueError, match="gdl_scene_finish: null pointer"):
        checked.gdl_scene_finish(None, 5, 35, 0.5, None, None, None)
