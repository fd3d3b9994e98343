#!/usr/bin/env python
"""Generate tests/golden/upernet_scale_modules*.npz by running the REAL reference UperNetDecoder(scale_modules=True).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_scale_modules.py

Same pattern as tools/make_goldens.py: the reference is imported read-only through tools/oracle_shim.py and only arrays are
written.  Inputs travel by recipe: weights = oracle.procedural_state_dict(decoder, seed) (generic over state-dict keys; the
build's decoder has the same keys), the four [2,64,12,12] taps and the cotangent g come from `recipe_inputs` below, which the
tests restate from the JSON meta.  Stored, from the reference in f32: train-mode outputs of fpn1 / fpn2 / fpn4 and of the
decoder, fpn1.1's updated running statistics, eval-mode fpn1 / decoder outputs on a fixed stride, and the gradients of
sum(out * g) with respect to the four inputs and every fpn* parameter.  The float64 self-check of the gradient rule runs here
too (see tests/test_hip_scale_modules.py).  The cotangent is scaled by 2^-9 (a power of two: every gradient is the exactly scaled
one): the three ConvTranspose biases feed a train-mode BatchNorm (fpn1.0.bias its own, fpn1.3.bias / fpn2.0.bias the lateral
ConvModule's through a 1x1 convolution), their gradients are analytically zero and the reference's f32 rounding noise on them
grows with the cotangent (4.9e-5 for fpn1.0.bias at unit scale) -- at 2^-9 both sides can be held to 1e-6 like the neck's conv
biases.
Two files, because one committed file stays below 1 MiB: the decoder's train-mode
output lives in upernet_scale_modules_out.npz, everything else in upernet_scale_modules.npz.
"""

from __future__ import annotations

import copy
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT))
import oracle_shim  # noqa: E402

oracle_shim.install()

from oracle import procedural_state_dict  # noqa: E402

from geo_deep_learning.models.decoders.upernet import UperNetDecoder as RefUper  # noqa: E402

GOLD = ROOT / "tests" / "golden"
ZERO_GRAD = ("fpn1.0.bias", "fpn1.3.bias", "fpn2.0.bias")      # analytically zero: a per-channel constant in front of a train-mode BatchNorm
META = dict(seed=42, embed=64, channels=32, batch=2, size=12, eval_stride=3, input_std=1.0, g_std=2.0 ** -9)


def recipe_inputs(meta: dict):
    """Four taps [B, E, S, S] and the cotangent [B, channels, 4S, 4S]: standard normals of np.random.default_rng([seed, 2024, i])
    (i = 0..3 taps, 4 cotangent) as float32."""
    b, e, s, ch = meta["batch"], meta["embed"], meta["size"], meta["channels"]
    xs = [torch.from_numpy((np.random.default_rng([meta["seed"], 2024, i]).standard_normal((b, e, s, s)) * meta["input_std"])
                           .astype(np.float32)) for i in range(4)]
    g = torch.from_numpy((np.random.default_rng([meta["seed"], 2024, 4]).standard_normal((b, ch, 4 * s, 4 * s)) * meta["g_std"])
                         .astype(np.float32))
    return xs, g


def train_step(dec, xs, g):
    xs = [x.clone().requires_grad_(True) for x in xs]
    hooks = {}
    hs = [getattr(dec, n).register_forward_hook(lambda m, i, o, n=n: hooks.__setitem__(n, o.detach())) for n in ("fpn1", "fpn2", "fpn4")]
    out = dec(xs)
    (out * g.to(out.dtype)).sum().backward()
    for h in hs:
        h.remove()
    return out.detach(), hooks, [x.grad for x in xs]


def main() -> None:
    torch.manual_seed(META["seed"])
    e = META["embed"]
    ref = RefUper([e] * 4, channels=META["channels"], align_corners=False, scale_modules=True)
    keys = list(ref.state_dict().keys())
    sd = procedural_state_dict(ref, META["seed"])
    ref.load_state_dict(sd)
    xs, g = recipe_inputs(META)
    ref.train()
    out, hooks, dxs = train_step(ref, xs, g)
    res = dict(train_fpn1=hooks["fpn1"].numpy(), train_fpn2=hooks["fpn2"].numpy(), train_fpn4=hooks["fpn4"].numpy(),
               running_mean=ref.fpn1[1].running_mean.numpy().copy(), running_var=ref.fpn1[1].running_var.numpy().copy())
    for i, d in enumerate(dxs):
        res[f"grad_input{i}"] = d.numpy()
    fpn_names = [n for n, _ in ref.named_parameters() if n.split(".")[0] in ("fpn1", "fpn2", "fpn3", "fpn4")]
    for n, p in ref.named_parameters():
        if n in fpn_names:
            res["grad/" + n] = p.grad.numpy().copy()

    # the gradient rule of the decoder-level test, checked on the reference against itself in float64 (it must miss nothing)
    r64 = copy.deepcopy(ref).double()
    r64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()})
    r64.zero_grad()
    r64.train()
    _, _, dxs64 = train_step(r64, [x.double() for x in xs], g.double())
    worst = 0.0
    pairs = [(f"grad_input{i}", dxs[i], dxs64[i]) for i in range(4)]
    pairs += [(n, dict(ref.named_parameters())[n].grad, dict(r64.named_parameters())[n].grad) for n in fpn_names]
    for n, a, b in pairs:
        if n in ZERO_GRAD:
            assert a.norm() <= 1e-6 and b.norm() <= 1e-6, (n, a.norm(), b.norm())
            continue
        rn = b.norm().item()
        assert abs(a.double().norm().item() - rn) <= 2e-2 * rn + 2e-5, n
        bad = ((a.double() - b).abs() > 5 * 2e-2 * b.abs().max() + 1e-9).double().mean().item()
        worst = max(worst, bad)
    assert worst <= 0.01, worst
    print("f32 vs f64 reference: worst share of elements off", worst)

    ref.eval()
    st = META["eval_stride"]
    with torch.no_grad():
        res["eval_fpn1_s"] = ref.fpn1(xs[0])[:, :, 1::st, 1::st].contiguous().numpy()
        res["eval_out_s"] = ref(xs)[:, :, 1::st, 1::st].contiguous().numpy()
    meta = dict(META, keys=keys, shapes={k: list(v.shape) for k, v in sd.items()}, dtypes={k: str(v.dtype) for k, v in sd.items()},
                fpn_params=fpn_names, zero_grad=list(ZERO_GRAD), f64_worst_share_off=worst)
    res["meta"] = np.array(json.dumps(meta))
    GOLD.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(GOLD / "upernet_scale_modules.npz", **res)
    np.savez_compressed(GOLD / "upernet_scale_modules_out.npz", train_out=out.numpy())
    for f in ("upernet_scale_modules.npz", "upernet_scale_modules_out.npz"):
        print(f, (GOLD / f).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
