"""CPU-side checks of UperNetDecoder(scale_modules=True) (reference upernet.py:37-54,113-119): the module tree the build
constructs is the reference's (state-dict keys, shapes, dtypes as recorded from the real reference in the golden's meta), and the
golden files are arrays + a short JSON meta whose recipe the tests can restate."""

import json

import numpy as np
import torch
from torch import nn

from _scale_modules_recipe import load_golden, recipe_inputs
from geo_deep_learning.models.decoders.upernet import UperNetDecoder
from geo_deep_learning.models.utils import ConvModule
from oracle import procedural_state_dict


def test_state_dict_matches_the_reference_and_syncbn_converts():
    dec = UperNetDecoder([768] * 4, align_corners=False, scale_modules=True)
    sd = dec.state_dict()
    assert len(sd) == 83
    assert dec.embed_dim == [192, 384, 768, 768]
    assert tuple(sd["fpn1.0.weight"].shape) == (768, 384, 2, 2) and tuple(sd["fpn1.3.weight"].shape) == (384, 192, 2, 2)
    assert tuple(sd["fpn2.0.weight"].shape) == (768, 384, 2, 2) and tuple(sd["fpn1.1.running_var"].shape) == (384,)
    assert isinstance(dec.fpn3[0], nn.Identity) and isinstance(dec.fpn4[0], nn.MaxPool2d)
    # the key list / shapes / dtypes recorded from the REAL reference (small dims) against the build at the same dims
    meta = load_golden()[1]
    small = UperNetDecoder([meta["embed"]] * 4, channels=meta["channels"], align_corners=False, scale_modules=True)
    ssd = small.state_dict()
    assert list(ssd.keys()) == meta["keys"] == list(sd.keys()) and len(meta["keys"]) == 83
    for k, v in ssd.items():
        assert list(v.shape) == meta["shapes"][k] and str(v.dtype) == meta["dtypes"][k], k
    conv = nn.SyncBatchNorm.convert_sync_batchnorm(dec)
    assert isinstance(conv.fpn1[1], nn.SyncBatchNorm) and isinstance(conv.fpn1[0], nn.ConvTranspose2d)


def test_unsupported_switches_keep_raising():
    import pytest
    with pytest.raises(NotImplementedError):
        UperNetDecoder([64] * 4, align_corners=True, scale_modules=True)
    with pytest.raises(NotImplementedError):
        ConvModule(8, 8, 2, transpose=True)


def test_golden_is_arrays_plus_recipe():
    gold, meta = load_golden()
    for k in gold.files:
        assert gold[k].dtype.kind in "fU", (k, gold[k].dtype)          # float arrays and the JSON string only
    assert meta["seed"] == 42 and (meta["batch"], meta["embed"], meta["size"], meta["channels"]) == (2, 64, 12, 32)
    assert len(json.dumps({k: meta[k] for k in meta if k not in ("keys", "shapes", "dtypes")})) < 600
    xs, g = recipe_inputs(meta)
    assert [tuple(x.shape) for x in xs] == [(2, 64, 12, 12)] * 4 and tuple(g.shape) == (2, 32, 48, 48)
    assert gold["train_fpn1"].shape == (2, 16, 48, 48) and gold["train_fpn2"].shape == (2, 32, 24, 24)
    assert gold["train_fpn4"].shape == (2, 64, 6, 6) and gold["train_out"].shape == (2, 32, 48, 48)
    for i in range(4):
        assert gold[f"grad_input{i}"].shape == (2, 64, 12, 12)
    dec = UperNetDecoder([64] * 4, channels=32, align_corners=False, scale_modules=True)
    sd = procedural_state_dict(dec, meta["seed"])
    for n in meta["fpn_params"]:
        assert gold["grad/" + n].shape == tuple(sd[n].shape), n
    assert set(meta["fpn_params"]) == {n for n, _ in dec.named_parameters() if n.split(".")[0] in ("fpn1", "fpn2")}
    # the max-pool level is plain data movement: the golden is reproduced bit for bit from the recipe on the CPU
    want = torch.nn.functional.max_pool2d(xs[3], 2, 2).numpy()
    assert np.array_equal(gold["train_fpn4"], want)
    assert meta["f64_worst_share_off"] <= 0.01
