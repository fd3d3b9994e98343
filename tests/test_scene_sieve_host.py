"""Host side of the sieve for whole-scene inference, no GPU: the binding of include/gdlhip_scene_sieve.h (SCENE_SIEVE_SIGNATURES)
beside the five other sets, the argument checks of its entry points and of ``gdlhip.ops`` / ``SceneInference``, which fire before
anything touches a device, and the numpy restatement the GPU tests compare with (tests/_sieve_oracle.py): against
``scipy.ndimage.label`` for the components and against results written out by hand for the sieve."""

import ctypes as C

import numpy as np
import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
import _sieve_oracle as so  # noqa: E402
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402
from geo_deep_learning.tools.scene_inference import SceneInference  # noqa: E402
from geo_deep_learning.tools.script_model import ScriptModel  # noqa: E402

NAMES = ["gdl_scene_components", "gdl_scene_sieve"]


def test_sieve_header_is_bound_beside_the_other_sets():
    i, p = C.c_int, C.c_void_p
    sig = _lib.SCENE_SIEVE_SIGNATURES
    assert sorted(sig) == NAMES
    assert sig["gdl_scene_components"] == (i, [p, i, i, i, i, p, p, p])
    assert sig["gdl_scene_sieve"] == (i, [p, p, p, i, i, i, i, i, p, p, p])
    for other in (_lib.SIGNATURES, _lib.DEBUG_SIGNATURES, _lib.SCENE_SIGNATURES, _lib.SCENE_TTA_SIGNATURES, _lib.SCENE_NODATA_SIGNATURES):
        assert not set(sig) & set(other)
    assert not set(sig) & _lib.STATUS_FUNCTIONS and set(sig) <= _lib._CHECKED
    # the existing scene sets keep their sizes
    assert len(_lib.SCENE_SIGNATURES) == 4 and len(_lib.SCENE_TTA_SIGNATURES) == 3 and len(_lib.SCENE_NODATA_SIGNATURES) == 4


def test_sieve_functions_are_exported_and_status_checked():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    raw, checked = _lib.load(), _lib.checked()
    for n, (res, args) in _lib.SCENE_SIEVE_SIGNATURES.items():
        assert getattr(raw, n).argtypes == args and getattr(raw, n).restype is res
        assert getattr(checked, n).errcheck is _lib.status_errcheck
    # a bad argument needs no device: the status comes back in load(), an exception in checked()
    null = {
        "gdl_scene_components": (None, 37, 53, 4, -1, None, None, None),
        "gdl_scene_sieve": (None, None, None, 37, 53, 4, 9, -1, None, None, None),
    }
    assert sorted(null) == NAMES
    for name, args in null.items():
        assert getattr(raw, name)(*args) == -1
        assert f"{name}: null pointer".encode() in raw.gdl_last_error()
        with pytest.raises(ValueError, match=f"{name}: null pointer"):
            getattr(checked, name)(*args)
    # one null pointer among the others is enough
    buf = (C.c_char * 64)()
    a = C.addressof(buf)
    assert raw.gdl_scene_components(a, 4, 4, 4, -1, a, None, None) == -1 and b"gdl_scene_components: null pointer" in raw.gdl_last_error()
    assert raw.gdl_scene_sieve(a, a, a, 4, 4, 4, 2, -1, None, a, None) == -1 and b"gdl_scene_sieve: null pointer" in raw.gdl_last_error()
    # the other argument checks come before any launch too: the pointers below are never followed
    calls = {
        "gdl_scene_components": lambda H, W, conn, ign: raw.gdl_scene_components(a, H, W, conn, ign, a, a, None),
        "gdl_scene_sieve": lambda H, W, conn, ign: raw.gdl_scene_sieve(a, a, a, H, W, conn, 2, ign, a, a, None),
    }
    for name, call in calls.items():
        for conn in (6, 0, 5):
            assert call(4, 4, conn, -1) == -1 and f"{name}: connectivity {conn} is neither 4 nor 8".encode() in raw.gdl_last_error()
        for ign in (-2, 256):
            assert call(4, 4, 4, ign) == -1 and f"{name}: ignore_label {ign} is not in -1..255".encode() in raw.gdl_last_error()
        for H, W in ((65536, 32768), (2, 2 ** 30), (46341, 46341)):      # H * W >= 2^31
            assert H * W >= 2 ** 31
            assert call(H, W, 4, -1) == -1
            assert f"{name}: {H} x {W} pixels".encode() in raw.gdl_last_error() and b"2^31" in raw.gdl_last_error()
        for H, W in ((0, 4), (4, 0), (-1, 4)):
            assert call(H, W, 4, -1) == -1 and f"{name}: bad sizes".encode() in raw.gdl_last_error()
    with pytest.raises(ValueError, match="gdl_scene_components: connectivity 6"):
        checked.gdl_scene_components(a, 4, 4, 6, -1, a, a, None)


# ------------------------------------------------------------------ the numpy restatement against scipy
SHAPES = [(70, 45), (37, 53), (1, 40), (40, 1), (1, 1)]


def _scipy_components(ndimage, mask: np.ndarray, connectivity: int, ignore_label: int):
    """scipy's labels, one class at a time, renamed to the smallest linear index of each component."""
    H, W = mask.shape
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)      # the cross / the full 3 x 3
    index = np.arange(H * W).reshape(H, W)
    labels = np.full((H, W), -1, dtype=np.int32)
    for value in np.unique(mask):
        if value == ignore_label:
            continue
        lab, n = ndimage.label(mask == value, structure=structure)
        smallest = np.full(n + 1, H * W, dtype=np.int64)
        np.minimum.at(smallest, lab.ravel(), index.ravel())
        labels = np.where(lab > 0, smallest[lab], labels).astype(np.int32)
    sizes = np.bincount(labels[labels >= 0], minlength=H * W).astype(np.int32)
    return labels, sizes


@pytest.mark.parametrize("name", list(so.patterns(16)))
def test_the_oracle_agrees_with_scipy(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    make, ignore = so.patterns(16)[name]
    for H, W in SHAPES:
        mask = make(H, W)
        for connectivity in (4, 8):
            for ign in (-1, ignore):
                labels, sizes = so.components(mask, connectivity, ign)
                want_labels, want_sizes = _scipy_components(ndimage, mask, connectivity, ign)
                assert labels.dtype == np.int32 and sizes.dtype == np.int32 and sizes.shape == (H * W,)
                assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes), (name, H, W, connectivity, ign)
                assert int(sizes.sum()) == int((mask != ign).sum())


def test_the_patterns_are_what_their_names_say():
    p = so.patterns(16)
    arm = p["spiral"][0](70, 45)
    for connectivity in (4, 8):      # one arm and one gap, each a single component that winds through the whole mask
        labels, sizes = so.components(arm, connectivity)
        assert len(np.unique(labels)) == 2 and sizes[0] == arm.sum() and 0 < arm.sum() < arm.size
    board = p["checkerboard"][0](37, 53)
    assert (so.components(board, 4)[1] == 1).all() and (so.components(board, 8)[1] > 0).sum() == 2
    assert so.components(p["constant"][0](37, 53), 4)[1][0] == 37 * 53
    cross = p["ignore-cross"][0](37, 53)
    assert (cross[16] == 255).all() and (cross[:, 15] == 255).all() and (so.components(cross, 4, 255)[0][16] == -1).all()
    lines = p["diagonal-lines"][0](37, 53)
    assert (so.components(lines, 4)[1][lines.ravel() == 1] == 1).all() and (so.components(lines, 8)[1] > 1).sum() > 10


# ------------------------------------------------------------------ the sieve by hand
@pytest.mark.parametrize("name,mask,kw,want", so.HAND_CASES, ids=[c[0] for c in so.HAND_CASES])
def test_the_oracle_sieve_on_hand_drawn_cases(name, mask, kw, want):
    assert mask.shape == (5, 7) and want.shape == (5, 7)
    before = mask.copy()
    got = so.sieve(mask, **kw)
    assert got.dtype == np.uint8 and np.array_equal(got, want), f"\n{got}"
    assert np.array_equal(mask, before)


def test_the_oracle_sieve_identities():
    mask = so.patterns()["random-5"][0](37, 53)
    for connectivity in (4, 8):
        for min_size in (-3, 0, 1, 37 * 53 + 1):      # nothing is small; everything is
            assert np.array_equal(so.sieve(mask, min_size, connectivity), mask)
        once = so.sieve(mask, 4, connectivity)
        assert not np.array_equal(once, mask)
        assert np.array_equal(so.sieve(mask, 4, connectivity, iterations=3), so.sieve(so.sieve(once, 4, connectivity), 4, connectivity))
        # ignored pixels are never changed and their value is never handed out
        ign = so.sieve(mask, 4, connectivity, ignore_label=2)
        assert np.array_equal(ign == 2, mask == 2) and not np.array_equal(ign, mask)


# ------------------------------------------------------------------ the argument checks of ops and SceneInference
def test_ops_check_their_arguments_before_a_device_is_needed():
    mask = torch.zeros((5, 7), dtype=torch.uint8)
    for fn, args in ((ops.scene_components, ()), (ops.scene_sieve, (3,))):
        op = fn.__name__
        with pytest.raises(ValueError, match=f"{op}: contiguous uint8 / bool \\[H, W\\] mask expected, got torch.int64"):
            fn(mask.long(), *args)
        with pytest.raises(ValueError, match=f"{op}: contiguous uint8 / bool \\[H, W\\] mask expected"):
            fn(mask[None], *args)
        with pytest.raises(ValueError, match=f"{op}: contiguous uint8 / bool"):
            fn(mask.t(), *args)
        with pytest.raises(ValueError, match=f"{op}: connectivity must be 4 or 8, got 6"):
            fn(mask, *args, connectivity=6)
        for bad in (-1, 256, 1.0, True):
            with pytest.raises(ValueError, match=f"{op}: ignore_label must be None or an int in 0..255"):
                fn(mask, *args, ignore_label=bad)
        with pytest.raises(ValueError, match=f"{op}: empty mask"):
            fn(torch.zeros((0, 7), dtype=torch.uint8), *args)
        with pytest.raises(ValueError, match="device tensors"):
            fn(mask, *args)
        with pytest.raises(ValueError, match="device tensors"):
            fn(mask.bool(), *args)
    for bad in (2.0, None, True):
        with pytest.raises(ValueError, match="scene_sieve: min_size must be an int"):
            ops.scene_sieve(mask, bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="scene_sieve: iterations must be an int of at least 1"):
            ops.scene_sieve(mask, 3, iterations=bad)


def _si(**kw) -> SceneInference:
    sm = ScriptModel(torch.nn.Identity(), device=torch.device("cpu"), num_classes=2, input_shape=(1, 3, 16, 16))
    return SceneInference(sm, tile=(16, 16), **kw)


@pytest.mark.parametrize("kw,match", [
    (dict(sieve=0), "sieve must be None or a pixel count of at least 1, got 0"),
    (dict(sieve=-4), "sieve must be None or a pixel count of at least 1, got -4"),
    (dict(sieve=2.5), "sieve must be None or a pixel count of at least 1"),
    (dict(sieve=True), "sieve must be None or a pixel count of at least 1"),
    (dict(sieve_connectivity=6), "sieve_connectivity must be 4 or 8, got 6"),
    (dict(sieve_connectivity="8"), "sieve_connectivity must be 4 or 8"),
    (dict(sieve_connectivity=True), "sieve_connectivity must be 4 or 8"),
    (dict(sieve_iterations=0), "sieve_iterations must be an int of at least 1, got 0"),
    (dict(sieve_iterations=1.0), "sieve_iterations must be an int of at least 1"),
    (dict(sieve=9, sieve_iterations=-1), "sieve_iterations must be an int of at least 1, got -1"),
], ids=str)
def test_scene_inference_rejects_at_construction(kw, match):
    with pytest.raises(ValueError, match="SceneInference: " + match):
        _si(**kw)


def test_scene_inference_defaults_are_off():
    si = _si()
    assert si.sieve is None and si.sieve_connectivity == 4 and si.sieve_iterations == 1
    on = _si(sieve=25, sieve_connectivity=8, sieve_iterations=2)
    assert on.sieve == 25 and on.sieve_connectivity == 8 and on.sieve_iterations == 2
