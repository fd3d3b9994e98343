"""GPU tests of burning polygon rings into a label raster: ``ops.scene_burn`` (include/gdlhip_scene_burn.h),
``rings_agreement`` and ``SceneInference.predict_rings(agreement=True)``.

Every comparison is exact, counts included.  The yardstick is the integer restatement of tests/_burn_oracle.py (which
tests/test_scene_burn_host.py holds against results written out by hand and against the ring tracer's round trip), computed
once per input and shared.  Shapes: the row kernel resolves GDL_SCENE_BURN_CHUNK = 256 pixels of a row per turn, a wave 64 of
them, so W in 63, 64, 65, 255, 256, 257 and 513 straddles the wave and the chunk boundaries (one, two and three turns with a
carry), H in 5 and 37 gives several workgroups, and 1 x 1, 1 x W and H x 1 are the degenerate rasters.  The 70 x 300 mask of
three random classes has some 28 000 crossings: more than a dozen scan tiles of 2048."""

import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
import _burn_oracle as bo  # noqa: E402
import _rings_oracle as ro  # noqa: E402
import _sieve_oracle as so  # noqa: E402
import oracle  # noqa: E402
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402
from gdlhip import scene as gscene  # noqa: E402
from geo_deep_learning.models.encoders.dofa_v2 import DOFAv2  # noqa: E402
from geo_deep_learning.models.segmentation.dofa import DOFASegmentationModel  # noqa: E402
from geo_deep_learning.tools.scene_inference import (SceneFeatures, SceneFeaturesAgreement, SceneInference, SceneVectors,  # noqa: E402
                                                      SceneVectorsAgreement, rings_agreement)
from geo_deep_learning.tools.script_model import SegmentationScriptModel  # noqa: E402
from oracle import procedural_state_dict, synthetic_batch  # noqa: E402
from oracle.model import RGB_MEAN, RGB_STD  # noqa: E402

DEV = "cuda"
SHAPES = [(1, 1), (1, 300), (300, 1)] + [(h, w) for h in (5, 37) for w in (63, 64, 65, 255, 256, 257, 513)]
shape_ids = [f"{h}x{w}" for h, w in SHAPES]


@functools.lru_cache(maxsize=None)
def _mask(H: int, W: int, classes: int = 3, seed: int = 5) -> np.ndarray:
    m = np.random.default_rng([seed, H, W]).integers(0, classes, (H, W)).astype(np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _traced(H: int, W: int, connectivity: int = 4, ignore: int = -1, values=None) -> ro.Rings:
    return ro.trace(_mask(H, W), connectivity, ignore, values)


def _dev(rings) -> gscene.FeatureRings:
    return gscene.FeatureRings(*(torch.from_numpy(np.ascontiguousarray(f)) for f in (rings.vertices, rings.ring_offsets, rings.value))).to(DEV)


def _same(got: ops.SceneBurn, want: bo.Burn) -> bool:
    assert isinstance(got, ops.SceneBurn) and got.mask.dtype == torch.uint8 and got.mask.is_cuda
    return np.array_equal(got.mask.cpu().numpy(), want.mask) and got.conflicts == want.conflicts and got.differ == want.differ


# ------------------------------------------------------------------ 1. ops.scene_burn against the oracle
@pytest.mark.parametrize("H,W", SHAPES, ids=shape_ids)
def test_traced_rings_burn_back_to_the_mask(H, W):
    mask, rings = _mask(H, W), _traced(H, W)
    want = bo.burn(rings, H, W, background=200, conflict=201, reference=mask)
    assert want.conflicts == 0 and want.differ == 0 and np.array_equal(want.mask, mask)
    got = ops.scene_burn(_dev(rings), (H, W), background=200, conflict=201, reference=torch.from_numpy(mask.copy()).to(DEV))
    assert _same(got, want)
    # shifted by a third of the raster both ways: clipped on every side, conflicts where the copies overlap
    both = bo.Rings(np.concatenate([rings.vertices, rings.vertices + np.array([W // 3 + 1, -(H // 3)], dtype=np.int32)]),
                    np.concatenate([rings.ring_offsets, rings.ring_offsets[1:] + len(rings.vertices)]),
                    np.concatenate([rings.value, rings.value + 1]))
    other = np.roll(mask, 1, axis=1)
    want = bo.burn(both, H, W, conflict=9, reference=other)
    assert _same(ops.scene_burn(_dev(both), (H, W), conflict=9, reference=torch.from_numpy(other).to(DEV)), want)
    assert W < 3 or want.conflicts > 0


def test_many_scan_tiles_and_two_runs_give_the_same_bits():
    H, W = 70, 300
    mask, rings = _mask(H, W), _traced(H, W)
    assert len(bo.crossings(rings, H, W)) > 6 * _lib.SCENE_BURN_SCAN_TILE and len(rings.vertices) > 6 * _lib.SCENE_BURN_SCAN_TILE
    dev = _dev(rings)
    first, second = ops.scene_burn(dev, (H, W), background=7), ops.scene_burn(dev, (H, W), background=7)
    assert _same(first, bo.burn(rings, H, W, background=7)) and torch.equal(first.mask, second.mask) and first[1:] == second[1:]
    assert first.differ is None and np.array_equal(first.mask.cpu().numpy(), mask)
    # the order of the rings does not matter
    order = np.random.default_rng(3).permutation(len(rings.value))
    lists = [rings.vertices[rings.ring_offsets[r]:rings.ring_offsets[r + 1]] for r in order]
    shuffled = bo.Rings(np.concatenate(lists), np.cumsum([0] + [len(v) for v in lists]).astype(np.int32), rings.value[order])
    assert torch.equal(ops.scene_burn(_dev(shuffled), (H, W), background=7).mask, first.mask)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_round_trip_from_scene_rings(connectivity):
    H, W = 37, 257
    mask = torch.from_numpy(_mask(H, W, 4).copy()).to(DEV)
    rings = ops.scene_rings(mask, connectivity)
    got = ops.scene_burn(rings, (H, W), background=77, reference=mask)
    assert torch.equal(got.mask, mask) and got.conflicts == 0 and got.differ == 0
    # values= plus a background: the classes left out, holes whose islands are missing included
    some = ops.scene_burn(ops.scene_rings(mask, connectivity, values=[1, 3]), (H, W), background=9, reference=mask)
    want = torch.where((mask == 1) | (mask == 3), mask, torch.full_like(mask, 9))
    assert torch.equal(some.mask, want) and some.conflicts == 0 and some.differ == int((want != mask).sum())
    # ignore_label: those pixels have no ring
    part = ops.scene_burn(ops.scene_rings(mask, connectivity, ignore_label=2), (H, W), background=2, reference=mask)
    assert torch.equal(part.mask, mask) and part.conflicts == 0 and part.differ == 0


@pytest.mark.parametrize("tolerance", [0, 0.5, 1, 2.5, 8])
def test_simplified_rings_against_the_oracle(tolerance):
    H, W = 37, 257
    host = so.patterns(16)["percolation"][0](H, W)
    mask = torch.from_numpy(host).to(DEV)
    rings = ops.scene_rings_simplify(ops.scene_rings(mask, 4), mask, tolerance)
    got = ops.scene_burn(rings, (H, W), reference=mask)
    want = bo.burn(bo.Rings(*(f.cpu().numpy() for f in (rings.vertices, rings.ring_offsets, rings.value))), H, W, reference=host)
    print(f"tolerance {tolerance}: {want.conflicts} conflicts, {want.differ} of {H * W} pixels differ")
    assert _same(got, want)
    if tolerance == 0:
        assert got.conflicts == 0 and got.differ == 0 and torch.equal(got.mask, mask)


@pytest.mark.parametrize("name,rings,bits,kw,want,conflicts", bo.HAND_CASES, ids=[c[0] for c in bo.HAND_CASES])
def test_hand_drawn_cases(name, rings, bits, kw, want, conflicts):
    H, W = want.shape
    for shift in (0, 1, 8 - bits):
        got = ops.scene_burn(_dev(bo.make(rings, 1 << shift)), (H, W), bits=bits + shift, reference=torch.from_numpy(want).to(DEV), **kw)
        assert np.array_equal(got.mask.cpu().numpy(), want) and got.conflicts == conflicts and got.differ == 0, (shift, got)


@pytest.mark.parametrize("seed", range(3))
def test_a_fan_of_triangles_in_q8(seed):
    for H, W in ((37, 65), (5, 513)):
        rings = bo.fan(H, W, seed)
        got = ops.scene_burn(_dev(rings), (H, W), bits=8)
        assert _same(got, bo.burn(rings, H, W, bits=8)) and got.conflicts == 0 and int(got.mask.min()) >= 1


def test_no_rings_and_no_crossings():
    H, W = 5, 300
    ref = torch.from_numpy(_mask(H, W).copy()).to(DEV)
    empty = gscene.rings_from_features([]).to(DEV)
    got = ops.scene_burn(empty, (H, W), background=1, reference=ref)
    assert (got.mask == 1).all() and got.conflicts == 0 and got.differ == int((ref != 1).sum())
    assert ops.scene_burn(empty, (H, W)).differ is None
    # rings, but none that crosses a row of the raster: below it, flat, or of two vertices
    none = bo.make([(3, [(0, 9), (4, 9), (4, 12)]), (4, [(0, 1), (5, 1), (9, 1)]), (5, [(0, 0), (3, 3)])])
    got = ops.scene_burn(_dev(none), (H, W), background=0, reference=ref)
    assert (got.mask == 0).all() and got.conflicts == 0 and got.differ == int((ref != 0).sum())


def test_bad_rings_raise_and_launch_no_fill(monkeypatch):
    H, W = 5, 65
    rings = _traced(H, W)
    calls = []
    real = _lib.checked().gdl_scene_burn_fill
    monkeypatch.setattr(_lib.checked(), "gdl_scene_burn_fill", lambda *a: calls.append(a) or real(*a))
    far = rings.vertices.copy()
    far[7, 0] = 2 ** 20 + 1
    with pytest.raises(ValueError, match="scene_burn: 1 bad entries in the rings"):
        ops.scene_burn(_dev(rings._replace(vertices=far)), (H, W))
    far[7, 0], far[9, 1] = -2 ** 21 - 1, 2 ** 30
    with pytest.raises(ValueError, match="scene_burn: 2 bad entries in the rings"):
        ops.scene_burn(_dev(rings._replace(vertices=far)), (H, W), bits=1)
    for k, v, n in ((2, int(rings.ring_offsets[1]) - 1, 1), (0, -1, 1), (len(rings.value), len(rings.vertices) + 1, 1), (1, 2 ** 30, 2)):
        off = rings.ring_offsets.copy()
        off[k] = v
        assert bo.bad_entries(rings._replace(ring_offsets=off)) == n
        with pytest.raises(ValueError, match=f"scene_burn: {n} bad entries in the rings"):
            ops.scene_burn(_dev(rings._replace(ring_offsets=off)), (H, W))
    assert not calls
    edge = rings.vertices.copy()
    edge[7, 0] = 2 ** 20      # the bound itself is in range
    ops.scene_burn(_dev(rings._replace(vertices=edge)), (H, W))
    assert len(calls) == 1
    with pytest.raises(ValueError, match="scene_burn: the reference is on cpu"):
        ops.scene_burn(_dev(rings), (H, W), reference=torch.zeros((H, W), dtype=torch.uint8))


# ------------------------------------------------------------------ 2. SceneInference, DOFA, end to end
@pytest.fixture(scope="module")
def dofa(golden_dir):
    """The tiny DOFA recipe and the uint8 scene [3, 3 img, 2 img] of tests/test_hip_scene_regions.py, five classes."""
    meta = json.loads(str(np.load(golden_dir / "dofa_tiny.npz")["meta"]))
    nc, img = 5, meta["img"]
    ref = oracle.DOFASegmentationModel("dofa_tiny_test", (img, img), num_classes=nc, _encoder_kwargs=meta["tiny"], freeze_layers=["encoder"])
    sd = procedural_state_dict(ref, meta["seed"])
    model = DOFASegmentationModel(DOFAv2(img_size=img, pretrained=False, **meta["tiny"]), (img, img), num_classes=nc, pretrained=False,
                                  freeze_layers=["encoder"])
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    batch = synthetic_batch(2, 3, img, nc, meta["seed"])
    kw = dict(wavelengths=batch["wavelengths"], device=torch.device(DEV), num_classes=nc, input_shape=(1, 3, img, img), mean=RGB_MEAN, std=RGB_STD)
    sm = SegmentationScriptModel(model, **kw)
    scene = torch.randint(1, 256, (3, 3 * img, 2 * img), generator=torch.Generator().manual_seed(meta["seed"]), dtype=torch.uint8)
    scene[:, :3 * img // 2, :img] = 0
    return nc, SceneInference(sm, tile=(img, img), overlap=0.5, batch_size=64, fill=0, sieve=25), scene


def test_predict_rings_with_agreement(dofa):
    nc, si, scene = dofa
    plain = si.predict_rings(scene)
    assert type(plain) is SceneVectors and plain._fields == ("mask", "rings")
    exact = si.predict_rings(scene, agreement=True)
    assert type(exact) is SceneVectorsAgreement and torch.equal(exact.mask, plain.mask)
    for name, a, b in zip(plain.rings._fields, plain.rings, exact.rings):
        assert torch.equal(a, b), name
    report = exact.agreement
    assert sorted(report) == ["conflicts", "differ", "iou_counts"] and report["differ"] == 0 and report["conflicts"] == 0
    same = ops.iou_counts(plain.mask.long()[None], plain.mask.long()[None], nc)[0]
    assert torch.equal(report["iou_counts"], same) and int(same[0].sum()) == plain.mask.numel()
    # simplified: the report is rings_agreement of the rings returned, which is the burn against the mask
    rough = si.predict_rings(scene, simplify=2.5, agreement=True)
    assert torch.equal(rough.mask, plain.mask) and rough.rings.vertices.shape[0] < plain.rings.vertices.shape[0]
    by_hand = rings_agreement(rough.mask, rough.rings, nc)
    H, W = rough.mask.shape
    burn = ops.scene_burn(rough.rings, (H, W), reference=rough.mask)
    host = bo.burn(bo.Rings(*(f.cpu().numpy() for f in (rough.rings.vertices, rough.rings.ring_offsets, rough.rings.value))), H, W,
                   reference=rough.mask.cpu().numpy())
    assert _same(burn, host)
    counts = ops.iou_counts(burn.mask.long()[None], rough.mask.long()[None], nc)[0]
    for report in (rough.agreement, by_hand):
        assert report["differ"] == burn.differ == host.differ > 0 and report["conflicts"] == burn.conflicts
        assert torch.equal(report["iou_counts"], counts)
    assert int(counts[0].sum()) == H * W - burn.differ      # every pixel that agrees is an intersection of its class
    feats = si.predict_features(scene, agreement=True)
    assert type(feats) is SceneFeaturesAgreement and feats.agreement["differ"] == 0 and type(si.predict_features(scene)) is SceneFeatures
