"""GPU tests of the sieve of whole-scene inference: ``ops.scene_components`` / ``ops.scene_sieve`` (include/gdlhip_scene_sieve.h) and
``SceneInference(sieve=...)``.

Every comparison is exact.  The yardstick is the numpy restatement of tests/_sieve_oracle.py (which tests/test_scene_sieve_host.py
holds against scipy and against results written out by hand), computed once per mask and shared; for ``SceneInference`` it is also
the project's own unsieved inference.  The kernels' tile is 64 x 64, so 197 x 131 and 131 x 197 are three tiles and a remainder
one way and two and a remainder the other; 37 x 53 is the odd pair of the other scene tests, inside one tile; 1 x W, H x 1 and
1 x 1 are the degenerate rasters (200: three tile edges along the one axis there is)."""

import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
import _sieve_oracle as so  # noqa: E402
import oracle  # noqa: E402
from gdlhip import ops  # noqa: E402
from geo_deep_learning.models.encoders.dofa_v2 import DOFAv2  # noqa: E402
from geo_deep_learning.models.segmentation.dofa import DOFASegmentationModel  # noqa: E402
from geo_deep_learning.tools.scene_inference import SceneInference  # noqa: E402
from geo_deep_learning.tools.script_model import SegmentationScriptModel  # noqa: E402
from oracle import procedural_state_dict, synthetic_batch  # noqa: E402
from oracle.model import RGB_MEAN, RGB_STD  # noqa: E402

DEV = "cuda"
TILE = 64
SHAPES = [(197, 131), (131, 197), (37, 53), (1, 200), (200, 1), (1, 1)]
PATTERNS = so.patterns(TILE)
RANDOM = ["random-2", "random-5", "percolation"]
CONNECTIVITY = [4, 8]
shape_ids = [f"{h}x{w}" for h, w in SHAPES]


@functools.lru_cache(maxsize=None)
def _mask(name: str, H: int, W: int) -> np.ndarray:
    m = PATTERNS[name][0](H, W)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _components(name: str, H: int, W: int, connectivity: int, ignore):
    """The oracle's (labels, sizes) of a pattern, computed once."""
    labels, sizes = so.components(_mask(name, H, W), connectivity, -1 if ignore is None else ignore)
    labels.setflags(write=False)
    sizes.setflags(write=False)
    return labels, sizes


def _ignores(name: str):
    return (None, PATTERNS[name][1])


# ------------------------------------------------------------------ 1. components
@pytest.mark.parametrize("H,W", SHAPES, ids=shape_ids)
@pytest.mark.parametrize("name", list(PATTERNS))
def test_labels_and_sizes_are_the_oracles(name, H, W):
    host = _mask(name, H, W)
    mask = torch.from_numpy(host.copy()).to(DEV)
    for connectivity in CONNECTIVITY:
        for ignore in _ignores(name):
            labels, sizes = ops.scene_components(mask, connectivity, ignore)
            assert labels.dtype == torch.int32 and tuple(labels.shape) == (H, W) and labels.is_contiguous()
            assert sizes.dtype == torch.int32 and tuple(sizes.shape) == (H * W,)
            want_labels, want_sizes = _components(name, H, W, connectivity, ignore)
            where = (name, H, W, connectivity, ignore)
            assert np.array_equal(labels.cpu().numpy(), want_labels), where
            assert np.array_equal(sizes.cpu().numpy(), want_sizes), where
            again = ops.scene_components(mask, connectivity, ignore)      # the same bits from run to run
            assert torch.equal(again[0], labels) and torch.equal(again[1], sizes), where
    assert np.array_equal(mask.cpu().numpy(), host), "the input is not modified"


def test_the_big_cases_are_what_they_are_meant_to_be():
    """The patterns must reach what they are for at the sizes tried here: a spiral arm that is one component crossing every tile
    edge, a constant mask counted as one component of H * W pixels, a checkerboard of single pixels."""
    H, W = SHAPES[0]
    arm = _mask("spiral", H, W)
    labels, sizes = _components("spiral", H, W, 4, None)
    assert sizes[0] == arm.sum() and len(np.unique(labels)) == 2
    # both the arm and the gap cross every tile edge several times, and the edges away from the rim dozens of times
    rows = [(int((arm[y] & arm[y - 1]).sum()), int(((1 - arm[y]) & (1 - arm[y - 1])).sum())) for y in range(TILE, H, TILE)]
    cols = [(int((arm[:, x] & arm[:, x - 1]).sum()), int(((1 - arm[:, x]) & (1 - arm[:, x - 1])).sum())) for x in range(TILE, W, TILE)]
    assert len(rows) == 3 and len(cols) == 2
    assert min(min(p) for p in rows + cols) >= 2 and max(rows)[0] > 60 and max(cols)[0] > 60
    got_labels, got_sizes = ops.scene_components(torch.from_numpy(arm.copy()).to(DEV), 4)
    assert int(got_sizes[0]) == int(arm.sum()) and int(got_labels[H - 1, 0]) == 0
    const = ops.scene_components(torch.full((H, W), 7, dtype=torch.uint8, device=DEV), 8)
    assert int(const[1][0]) == H * W and int(const[1].sum()) == H * W and not const[0].any()
    board = ops.scene_components(torch.from_numpy(_mask("checkerboard", H, W).copy()).to(DEV), 4)
    assert torch.equal(board[0].flatten(), torch.arange(H * W, dtype=torch.int32, device=DEV)) and (board[1] == 1).all()
    cross = _mask("ignore-cross", H, W)
    assert (cross[TILE] == 255).all() and (cross[:, TILE - 1] == 255).all()      # the arms lie on the two sides of a tile edge


def test_a_bool_mask_is_the_same_mask():
    H, W = 37, 53
    host = _mask("percolation", H, W)
    mask = torch.from_numpy(host.copy()).to(DEV)
    a, b = ops.scene_components(mask, 8), ops.scene_components(mask.bool(), 8)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    out = ops.scene_sieve(mask.bool(), 9, 8)
    assert out.dtype == torch.uint8 and torch.equal(out, ops.scene_sieve(mask, 9, 8))


# ------------------------------------------------------------------ 2. the sieve
@pytest.mark.parametrize("H,W", SHAPES, ids=shape_ids)
@pytest.mark.parametrize("name", list(PATTERNS))
def test_sieve_is_the_oracles(name, H, W):
    host = _mask(name, H, W)
    mask = torch.from_numpy(host.copy()).to(DEV)
    changed = 0
    for connectivity in CONNECTIVITY:
        for ignore in _ignores(name):
            comps = _components(name, H, W, connectivity, ignore)
            ign = -1 if ignore is None else ignore
            for min_size in (1, 2, 9, H * W + 1):
                for iterations in ((1, 3) if name in RANDOM and min_size in (2, 9) else (1,)):
                    got = ops.scene_sieve(mask, min_size, connectivity, ignore, iterations)
                    assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W) and got.data_ptr() != mask.data_ptr()
                    want = so.sieve(host, min_size, connectivity, ign, iterations, comps)
                    where = (name, H, W, connectivity, ignore, min_size, iterations)
                    assert np.array_equal(got.cpu().numpy(), want), where
                    if min_size in (1, H * W + 1):      # nothing is small; nothing is kept
                        assert np.array_equal(want, host), where
                    changed += int((want != host).sum())
                    assert torch.equal(ops.scene_sieve(mask, min_size, connectivity, ignore, iterations), got), where
    assert np.array_equal(mask.cpu().numpy(), host), "the input is not modified"
    if name in RANDOM + ["ignore-cross"] and H * W > 1000:
        assert changed > 0      # the sieve had something to do


@pytest.mark.parametrize("name,mask,kw,want", so.HAND_CASES, ids=[c[0] for c in so.HAND_CASES])
def test_sieve_on_the_hand_drawn_cases(name, mask, kw, want):
    got = ops.scene_sieve(torch.from_numpy(mask.copy()).to(DEV), **kw)
    assert np.array_equal(got.cpu().numpy(), want), f"\n{got.cpu().numpy()}"


def test_the_two_entry_points_compose_as_the_wrapper_does():
    """``scene_sieve`` is gdl_scene_components + gdl_scene_sieve; min_size <= 1 through the library is a copy as well."""
    from gdlhip import _lib
    H, W = 131, 197
    host = _mask("random-5", H, W)
    mask = torch.from_numpy(host.copy()).to(DEV)
    labels, sizes = ops.scene_components(mask, 8, 1)
    best = torch.empty(H * W, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for min_size, want in ((4, so.sieve(host, 4, 8, 1)), (1, host), (0, host), (-5, host)):
        out = torch.full_like(mask, 99)
        _lib.checked().gdl_scene_sieve(mask.data_ptr(), labels.data_ptr(), sizes.data_ptr(), H, W, 8, min_size, 1, best.data_ptr(),
                                       out.data_ptr(), stream)
        assert np.array_equal(out.cpu().numpy(), want), min_size


# ------------------------------------------------------------------ 3. SceneInference, DOFA, end to end
@pytest.fixture(scope="module", params=[5, 1], ids=["softmax5", "sigmoid1"])
def dofa(request, golden_dir):
    """The tiny DOFA recipe and the uint8 scene [3, 3 img, 2 img] of tests/test_hip_scene_nodata.py (values 1..255 with a block of
    zeros over rows 0 .. 1.5 img and columns 0 .. img) and, computed once, the plain inference of the scene (no sieve)."""
    meta = json.loads(str(np.load(golden_dir / "dofa_tiny.npz")["meta"]))
    nc, img = request.param, meta["img"]
    ref = oracle.DOFASegmentationModel("dofa_tiny_test", (img, img), num_classes=nc, _encoder_kwargs=meta["tiny"], freeze_layers=["encoder"])
    sd = procedural_state_dict(ref, meta["seed"])
    model = DOFASegmentationModel(DOFAv2(img_size=img, pretrained=False, **meta["tiny"]), (img, img), num_classes=nc, pretrained=False,
                                  freeze_layers=["encoder"])
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    batch = synthetic_batch(2, 3, img, max(nc, 2), meta["seed"])
    kw = dict(wavelengths=batch["wavelengths"], device=torch.device(DEV), num_classes=nc, input_shape=(1, 3, img, img), mean=RGB_MEAN, std=RGB_STD)
    sm = SegmentationScriptModel(model, **kw)
    scene = torch.randint(1, 256, (3, 3 * img, 2 * img), generator=torch.Generator().manual_seed(meta["seed"]), dtype=torch.uint8)
    scene[:, :3 * img // 2, :img] = 0
    plain = SceneInference(sm, tile=(img, img), overlap=0.5, batch_size=64).predict(scene, return_probs=True)
    return nc, img, sm, scene, plain


def _si(dofa, **kw) -> SceneInference:
    nc, img, sm, *_ = dofa
    return SceneInference(sm, tile=(img, img), overlap=0.5, **{"batch_size": 64, "fill": 0, **kw})


def _small_and_kept(mask: np.ndarray, n: int, connectivity: int, ignore: int = -1) -> None:
    """The mask holds components below and components of at least ``n`` pixels, so a sieve at ``n`` has work and a place to put it."""
    sizes = so.components(mask, connectivity, ignore)[1]
    assert ((sizes > 0) & (sizes < n)).any() and (sizes >= n).any(), np.unique(sizes)


SIEVE = 25      # pixels: the minimum mapping unit of the end-to-end cases


@pytest.mark.parametrize("connectivity,iterations", [(4, 1), (8, 1), (4, 2)])
def test_sieved_inference_is_the_sieve_of_the_plain_mask(dofa, connectivity, iterations):
    nc, img, sm, scene, plain = dofa
    host = plain.mask.cpu().numpy()
    _small_and_kept(host, SIEVE, connectivity)
    res = _si(dofa, sieve=SIEVE, sieve_connectivity=connectivity, sieve_iterations=iterations).predict(scene, return_probs=True)
    assert res.mask.dtype == torch.uint8 and tuple(res.mask.shape) == tuple(plain.mask.shape)
    assert torch.equal(res.mask, ops.scene_sieve(plain.mask, SIEVE, connectivity, None, iterations))
    want = so.sieve(host, SIEVE, connectivity, -1, iterations)
    assert np.array_equal(res.mask.cpu().numpy(), want) and (want != host).any()
    assert torch.equal(res.probs, plain.probs), "the sieve edits the map, not the probabilities"
    assert _si(dofa, sieve=SIEVE, sieve_connectivity=connectivity, sieve_iterations=iterations).predict(scene).probs is None


def test_sieved_inference_leaves_nodata_alone(dofa):
    nc, img, sm, scene, plain = dofa
    for label in (255, 7):
        unsieved = _si(dofa, nodata=0, nodata_label=label).predict(scene, return_probs=True)
        host = unsieved.mask.cpu().numpy()
        nodata = host == label
        assert nodata[:3 * img // 2, :img].all() and not nodata[3 * img // 2:].any() and not nodata[:, img:].any()
        _small_and_kept(host, SIEVE, 4, label)
        res = _si(dofa, nodata=0, nodata_label=label, sieve=SIEVE).predict(scene, return_probs=True)
        got = res.mask.cpu().numpy()
        assert np.array_equal(got == label, nodata), "no nodata pixel is changed and no valid pixel takes the label"
        assert np.array_equal(got, so.sieve(host, SIEVE, 4, label)) and (got != host).any()
        assert torch.equal(res.mask, ops.scene_sieve(unsieved.mask, SIEVE, 4, label))
        assert torch.equal(res.probs, unsieved.probs)
    # the same through a plane of the caller's
    valid = torch.ones(scene.shape[1:], dtype=torch.bool)
    valid[:3 * img // 2, :img] = False
    assert torch.equal(_si(dofa, sieve=SIEVE, nodata_label=7).predict(scene, valid=valid).mask, res.mask)


def test_without_sieve_nothing_changes(dofa):
    nc, img, sm, scene, plain = dofa
    off = _si(dofa, sieve=None, sieve_connectivity=8, sieve_iterations=3).predict(scene, return_probs=True)
    assert torch.equal(off.mask, plain.mask) and torch.equal(off.probs, plain.probs)
    one = _si(dofa, sieve=1).predict(scene)      # a minimum mapping unit of one pixel keeps every region
    assert torch.equal(one.mask, plain.mask)
