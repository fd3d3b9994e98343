"""GPU tests of the polygon rings of whole-scene inference: ``ops.scene_rings`` (include/gdlhip_scene_rings.h),
``SceneInference.predict_rings`` and ``gdlhip.scene.polygons`` on their results.

Every comparison is exact.  The yardstick is the sequential tracer of tests/_rings_oracle.py (which tests/test_scene_rings_host.py
holds against its own inverse, against scipy and against rings written out by hand), computed once per mask and shared.  Shapes
and patterns are those of tests/test_hip_scene_sieve.py, each pattern for a reason: the spiral at 197 x 131 is one ring of tens of
thousands of sides (more than a dozen doubling rounds), the checkerboard the dense bound (E = 4 H W sides, R = H W rings), the
constant mask one ring of four vertices, the rings pattern nested holes, percolation and random-5 the general case."""

import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
import _rings_oracle as ro  # noqa: E402
import _sieve_oracle as so  # noqa: E402
import oracle  # noqa: E402
from gdlhip import ops  # noqa: E402
from gdlhip import scene as gscene  # noqa: E402
from geo_deep_learning.models.encoders.dofa_v2 import DOFAv2  # noqa: E402
from geo_deep_learning.models.segmentation.dofa import DOFASegmentationModel  # noqa: E402
from geo_deep_learning.tools.scene_inference import SceneInference  # noqa: E402
from geo_deep_learning.tools.script_model import SegmentationScriptModel  # noqa: E402
from oracle import procedural_state_dict, synthetic_batch  # noqa: E402
from oracle.model import RGB_MEAN, RGB_STD  # noqa: E402

DEV = "cuda"
SHAPES = [(197, 131), (131, 197), (37, 53), (1, 200), (200, 1), (1, 1)]
PATTERNS = so.patterns(64)
CONNECTIVITY = [4, 8]
FIELDS = {"vertices": torch.int32, "ring_offsets": torch.int32, "value": torch.uint8, "label": torch.int32, "start": torch.int32,
          "area2": torch.int64}
shape_ids = [f"{h}x{w}" for h, w in SHAPES]


@functools.lru_cache(maxsize=None)
def _mask(name: str, H: int, W: int) -> np.ndarray:
    m = PATTERNS[name][0](H, W)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _rings(name: str, H: int, W: int, connectivity: int, ignore, values) -> ro.Rings:
    """The oracle's rings of a pattern, computed once; ``values`` a tuple or None."""
    rings = ro.trace(_mask(name, H, W), connectivity, -1 if ignore is None else ignore, values)
    for a in rings:
        a.setflags(write=False)
    return rings


def _equal(got, want: ro.Rings, where) -> None:
    assert tuple(got._fields) == tuple(FIELDS), where
    R, V = len(want.value), len(want.vertices)
    for name, dtype in FIELDS.items():
        g = getattr(got, name)
        assert g.is_cuda and g.dtype == dtype and g.is_contiguous(), (name, where)
        assert tuple(g.shape) == {"vertices": (V, 2), "ring_offsets": (R + 1,)}.get(name, (R,)), (name, tuple(g.shape), where)
        assert np.array_equal(g.cpu().numpy(), getattr(want, name)), (name, where)


def _host(rings) -> ro.Rings:
    return ro.Rings(*(f.cpu().numpy() for f in rings))


# ------------------------------------------------------------------ 1. the rings of the patterns
@pytest.mark.parametrize("H,W", SHAPES, ids=shape_ids)
@pytest.mark.parametrize("name", list(PATTERNS))
def test_rings_are_the_oracles(name, H, W):
    host = _mask(name, H, W)
    mask = torch.from_numpy(host.copy()).to(DEV)
    for connectivity in CONNECTIVITY:
        for ignore in (None, PATTERNS[name][1]):
            for values in ((None, (1, 3)) if name == "random-5" else (None,)):
                where = (name, H, W, connectivity, ignore, values)
                got = ops.scene_rings(mask, connectivity, ignore, values)
                _equal(got, _rings(name, H, W, connectivity, ignore, values), where)
                again = ops.scene_rings(mask, connectivity, ignore, values)      # the same bits from run to run
                assert all(torch.equal(a, b) for a, b in zip(got, again)), where
    assert np.array_equal(mask.cpu().numpy(), host), "the input is not modified"


def test_the_big_cases_are_what_they_are_meant_to_be():
    H, W = SHAPES[0]
    arm = _rings("spiral", H, W, 4, 0, None)      # the arm alone: one ring
    sides = int(np.abs(np.diff(np.concatenate([arm.vertices, arm.vertices[:1]]), axis=0)).sum())
    assert len(arm.value) == 1 and sides > 2 ** 14, "a ring long enough for more than a dozen doubling rounds"
    board = ops.scene_rings(torch.from_numpy(_mask("checkerboard", H, W).copy()).to(DEV), 4)
    assert board.value.numel() == H * W and board.vertices.shape[0] == 4 * H * W and (board.area2 == 2).all()
    assert torch.equal(board.start, 4 * torch.arange(H * W, dtype=torch.int32, device=DEV))
    const = ops.scene_rings(torch.full((H, W), 7, dtype=torch.uint8, device=DEV), 8)
    assert const.vertices.tolist() == [[W, 0], [W, H], [0, H], [0, 0]] and const.area2.tolist() == [2 * H * W]
    nested = _rings("rings", H, W, 4, None, None)
    assert (nested.area2 < 0).sum() >= 60, "holes inside holes"


def test_labels_of_the_caller_and_a_bool_mask():
    H, W = 131, 197
    host = _mask("percolation", H, W)
    mask = torch.from_numpy(host.copy()).to(DEV)
    want = _rings("percolation", H, W, 8, None, None)
    _equal(ops.scene_rings(mask, 8, labels=ops.scene_components(mask, 8)[0]), want, "labels=")
    _equal(ops.scene_rings(mask.bool(), 8), want, "bool")


def test_no_live_pixel_gives_no_ring():
    mask = torch.full((37, 53), 7, dtype=torch.uint8, device=DEV)
    for kw in (dict(ignore_label=7), dict(values=[]), dict(values=[3], connectivity=8)):
        got = ops.scene_rings(mask, **kw)
        assert tuple(got.vertices.shape) == (0, 2) and got.ring_offsets.tolist() == [0], kw
        assert all(getattr(got, f).numel() == 0 and getattr(got, f).dtype == FIELDS[f] for f in ("value", "label", "start", "area2")), kw
        assert gscene.polygons(got) == []


def test_argument_errors():
    mask = torch.zeros((5, 7), dtype=torch.uint8, device=DEV)
    for bad in (dict(connectivity=6), dict(connectivity=True), dict(values=[256]), dict(values=[-1]), dict(values=[1.0]), dict(values=3),
                dict(values="12"), dict(values=[True]), dict(ignore_label=256),
                dict(labels=torch.zeros((7, 5), dtype=torch.int32, device=DEV)),
                dict(labels=torch.zeros((5, 7), dtype=torch.int64, device=DEV)),
                dict(labels=torch.zeros((5, 7), dtype=torch.int32))):
        with pytest.raises(ValueError):
            ops.scene_rings(mask, **bad)
    for host in (mask.cpu(), mask.float(), mask[None], mask.t()):
        with pytest.raises(ValueError):
            ops.scene_rings(host)


# ------------------------------------------------------------------ 2. SceneInference, DOFA, end to end
@pytest.fixture(scope="module", params=[5, 1], ids=["softmax5", "sigmoid1"])
def dofa(request, golden_dir):
    """The tiny DOFA recipe and the uint8 scene [3, 3 img, 2 img] of tests/test_hip_scene_sieve.py: values 1..255 with a block of
    zeros over rows 0 .. 1.5 img and columns 0 .. img."""
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
    return nc, img, sm, scene


def _si(dofa, **kw) -> SceneInference:
    nc, img, sm, scene = dofa
    return SceneInference(sm, tile=(img, img), overlap=0.5, **{"batch_size": 64, "fill": 0, "sieve": 25, **kw})


@pytest.mark.parametrize("connectivity", CONNECTIVITY)
def test_predict_rings_is_the_rings_of_the_predicted_mask(dofa, connectivity):
    nc, img, sm, scene = dofa
    si = _si(dofa)
    res = si.predict_rings(scene, connectivity=connectivity)
    assert tuple(res._fields) == ("mask", "rings")
    assert torch.equal(res.mask, si.predict(scene).mask)
    host = res.mask.cpu().numpy()
    labels, sizes = so.components(host, connectivity)
    _equal(res.rings, ro.trace(host, connectivity, labels=labels), connectivity)
    assert np.array_equal(ro.fill(_host(res.rings), *host.shape), labels)
    features = gscene.polygons(res.rings)
    assert [f["properties"]["label"] for f in features] == np.flatnonzero(sizes).tolist(), "one feature per component, by label"
    assert [f["properties"]["pixels"] for f in features] == sizes[sizes > 0].tolist()


def test_predict_rings_gives_nodata_no_ring(dofa):
    nc, img, sm, scene = dofa
    label = 7
    si = _si(dofa, nodata=0, nodata_label=label)
    res = si.predict_rings(scene)
    host = res.mask.cpu().numpy()
    assert torch.equal(res.mask, si.predict(scene).mask) and (host == label).any()
    assert not (res.rings.value == label).any()
    labels, sizes = so.components(host, 4, label)
    _equal(res.rings, ro.trace(host, 4, label, labels=labels), "nodata")
    assert np.array_equal(ro.fill(_host(res.rings), *host.shape), labels), "the nodata pixels lie in no ring"
    assert len(gscene.polygons(res.rings)) == int((sizes > 0).sum())
    # the same through a plane of the caller's, and a keep set on top
    valid = torch.ones(scene.shape[1:], dtype=torch.bool)
    valid[:3 * img // 2, :img] = False
    through = _si(dofa, nodata_label=label).predict_rings(scene, valid, values=[1])
    assert torch.equal(through.mask, res.mask)
    _equal(through.rings, ro.trace(host, 4, label, (1,), labels), "valid=, values=")
    # without a plane the label is a class like any other
    present = int(_si(dofa).predict(scene).mask[0, 0])
    assert (_si(dofa, nodata_label=present).predict_rings(scene).rings.value == present).any()
