"""Recipe of tests/golden/upernet_scale_modules*.npz (restated from tools/make_golden_scale_modules.py, which ran the real
reference): inputs and cotangent from the JSON meta, and a loader that presents the two files as one."""
import json
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"


class _Gold:
    def __init__(self, parts):
        self._d = {}
        for p in parts:
            self._d.update({k: p[k] for k in p.files})
        self.files = list(self._d)

    def __getitem__(self, k):
        return self._d[k]


def load_golden():
    parts = [np.load(GOLDEN / f) for f in ("upernet_scale_modules.npz", "upernet_scale_modules_out.npz")]
    gold = _Gold(parts)
    return gold, json.loads(str(gold["meta"]))


def recipe_inputs(meta):
    b, e, s, ch = meta["batch"], meta["embed"], meta["size"], meta["channels"]
    xs = [torch.from_numpy((np.random.default_rng([meta["seed"], 2024, i]).standard_normal((b, e, s, s)) * meta["input_std"])
                           .astype(np.float32)) for i in range(4)]
    g = torch.from_numpy((np.random.default_rng([meta["seed"], 2024, 4]).standard_normal((b, ch, 4 * s, 4 * s)) * meta["g_std"])
                         .astype(np.float32))
    return xs, g
