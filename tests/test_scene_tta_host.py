"""Host side of test-time augmentation for whole-scene inference, no GPU: the transform codes of gdlhip/scene.py (``d4_apply``,
``d4_inverse``, ``tta_codes``, ``plan_tta``) against torch, and the binding of include/gdlhip_scene_tta.h
(SCENE_TTA_SIGNATURES) beside the three other sets."""

import ctypes as C

import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import _lib  # noqa: E402
from gdlhip import scene as gscene  # noqa: E402


def _asymmetric(h: int, w: int) -> torch.Tensor:
    """[2, h, w] of distinct values: no symmetry of the square maps it to itself."""
    return torch.arange(2 * h * w, dtype=torch.float32).reshape(2, h, w)


# code -> the torch expression it names (1 = flip x, 2 = flip y, 4 = transpose, the transpose first)
NAMED = {
    0: lambda x: x,
    1: lambda x: x.flip(-1),
    2: lambda x: x.flip(-2),
    3: lambda x: torch.rot90(x, 2, (-2, -1)),
    4: lambda x: x.transpose(-2, -1),
    5: lambda x: torch.rot90(x, 3, (-2, -1)),
    6: lambda x: torch.rot90(x, 1, (-2, -1)),
    7: lambda x: x.transpose(-2, -1).flip(-2).flip(-1),
}


@pytest.mark.parametrize("g", range(8))
def test_d4_apply_is_the_named_torch_expression(g):
    x = _asymmetric(5, 5)
    assert torch.equal(gscene.d4_apply(x, g), NAMED[g](x))
    if not g & 4:
        y = _asymmetric(4, 7)
        got = gscene.d4_apply(y, g)
        assert tuple(got.shape) == (2, 4, 7) and torch.equal(got, NAMED[g](y))


def test_quarter_turns_are_codes_6_3_5():
    x = _asymmetric(5, 5)
    for k, g in ((1, 6), (2, 3), (3, 5)):
        assert torch.equal(gscene.d4_apply(x, g), torch.rot90(x, k, (-2, -1))), (k, g)
    assert torch.equal(gscene.d4_apply(x, 3), x.flip(-2).flip(-1))


@pytest.mark.parametrize("g", range(8))
def test_d4_inverse_undoes_the_transform(g):
    x = _asymmetric(5, 5)
    inv = gscene.d4_inverse(g)
    assert torch.equal(gscene.d4_apply(gscene.d4_apply(x, g), inv), x)
    assert torch.equal(gscene.d4_apply(gscene.d4_apply(x, inv), g), x)
    assert inv == (g if not g & 4 else 4 | (g & 1) << 1 | (g >> 1 & 1))
    if not g & 4:
        y = _asymmetric(4, 7)
        assert torch.equal(gscene.d4_apply(gscene.d4_apply(y, g), inv), y)


def test_the_eight_images_differ_pairwise():
    x = _asymmetric(5, 5)
    images = [gscene.d4_apply(x, g) for g in gscene.D4]
    for a in range(8):
        for b in range(a + 1, 8):
            assert not torch.equal(images[a], images[b]), (a, b)


def test_d4_helpers_reject_a_code_outside_0_to_7():
    with pytest.raises(ValueError, match="0..7"):
        gscene.d4_apply(_asymmetric(5, 5), 8)
    with pytest.raises(ValueError, match="0..7"):
        gscene.d4_inverse(-1)


def test_tta_codes_names_and_sequences():
    assert gscene.D4 == (0, 1, 2, 3, 4, 5, 6, 7) and gscene.FLIPS == (0, 1, 2, 3)
    assert gscene.tta_codes(None, (16, 16)) == (0,) and gscene.tta_codes("none", (16, 12)) == (0,)
    assert gscene.tta_codes("flips", (16, 16)) == gscene.FLIPS and gscene.tta_codes("flips", (16, 12)) == gscene.FLIPS
    assert gscene.tta_codes("d4", (16, 16)) == gscene.D4
    assert gscene.tta_codes([0, 6, 3], (16, 16)) == (0, 6, 3)      # the order given is kept
    assert gscene.tta_codes((2, 1), (16, 12)) == (2, 1)


@pytest.mark.parametrize("tta,tile,match", [
    ("d8", (16, 16), "unknown tta"),
    (3, (16, 16), "unknown tta"),
    ((0, 3, 3), (16, 16), "repeated"),
    ((0, 8), (16, 16), "0..7"),
    ((-1,), (16, 16), "0..7"),
    ((0, 1.0), (16, 16), "0..7"),
    ((), (16, 16), "0..7"),
    ("d4", (16, 12), "square tile"),
    ((0, 5), (16, 12), "square tile"),
], ids=["name", "scalar", "repeated", "above", "below", "float", "empty", "d4-16x12", "code5-16x12"])
def test_tta_codes_rejects(tta, tile, match):
    with pytest.raises(ValueError, match=match):
        gscene.tta_codes(tta, tile)


def test_plan_tta_is_tile_major_in_the_order_of_the_codes():
    plan = gscene.plan_tiles(16, 28, (16, 16), (8, 12))
    assert plan.tolist() == [[0, 0], [0, 12]]
    origins, xforms = gscene.plan_tta(plan, (0, 6, 3))
    assert origins.dtype == torch.int32 and xforms.dtype == torch.int32
    assert tuple(origins.shape) == (6, 2) and tuple(xforms.shape) == (6,) and origins.is_contiguous() and xforms.is_contiguous()
    assert origins.tolist() == [[0, 0], [0, 0], [0, 0], [0, 12], [0, 12], [0, 12]]
    assert xforms.tolist() == [0, 6, 3, 0, 6, 3]
    same, zero = gscene.plan_tta(plan, (0,))
    assert torch.equal(same, plan) and zero.tolist() == [0, 0]


def test_tta_header_is_bound_beside_the_other_sets():
    i, d, p = C.c_int, C.c_double, C.c_void_p
    sig = _lib.SCENE_TTA_SIGNATURES
    assert sorted(sig) == ["gdl_scene_blend_d4", "gdl_scene_blend_lowres_d4", "gdl_scene_cut_d4"]
    # each is its counterpart of SCENE_SIGNATURES with one more pointer (xforms) after origins
    assert sig["gdl_scene_cut_d4"] == (i, [p, i, i, i, i, p, p, i, i, i, i, p, i, i, d, d, p, p, p])
    assert sig["gdl_scene_blend_d4"] == (i, [p, i, i, i, i, p, p, p, p, p, i, i, i, i, i, i, p])
    assert sig["gdl_scene_blend_lowres_d4"] == (i, [p, i, i, i, i, i, i, p, p, p, p, p, i, i, i, i, i, i, p])
    for name, at in (("gdl_scene_cut", 6), ("gdl_scene_blend", 6), ("gdl_scene_blend_lowres", 8)):
        res, args = _lib.SCENE_SIGNATURES[name]
        assert sig[name + "_d4"] == (res, args[:at] + [p] + args[at:])
    for other in (_lib.SIGNATURES, _lib.DEBUG_SIGNATURES, _lib.SCENE_SIGNATURES):
        assert not set(sig) & set(other)
    assert not set(sig) & _lib.STATUS_FUNCTIONS
    # the existing sets keep their sizes
    assert len(_lib.SCENE_SIGNATURES) == 4


def test_tta_functions_are_exported_and_status_checked():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    raw, checked = _lib.load(), _lib.checked()
    for n, (res, args) in _lib.SCENE_TTA_SIGNATURES.items():
        assert getattr(raw, n).argtypes == args and getattr(raw, n).restype is res
        assert getattr(checked, n).errcheck is _lib.status_errcheck
    # a bad argument needs no device: the status comes back in load(), an exception in checked()
    null_blend = (None, 1, 5, 16, 16, None, None, None, None, None, 16, 16, 0, 16, 0, 16, None)
    assert raw.gdl_scene_blend_d4(*null_blend) == -1
    assert b"gdl_scene_blend_d4: null pointer" in raw.gdl_last_error()
    with pytest.raises(ValueError, match="gdl_scene_blend_d4: null pointer"):
        checked.gdl_scene_blend_d4(*null_blend)
    assert raw.gdl_scene_cut_d4(None, 0, 3, 37, 53, None, None, 1, 16, 16, 0, None, 0, 255, 0.0, 1.0, None, None, None) == -1
    assert b"gdl_scene_cut_d4: null pointer" in raw.gdl_last_error()
    assert raw.gdl_scene_blend_lowres_d4(None, 1, 4, 4, 5, 16, 16, None, None, None, None, None, 16, 16, 0, 16, 0, 16, None) == -1
    assert b"gdl_scene_blend_lowres_d4: null pointer" in raw.gdl_last_error()
