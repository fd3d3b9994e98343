"""Worker of tests/test_hip_soft_bce.py::test_graphed_soft_bce_step_reproduces_the_eager_losses_bit_for_bit: training steps of the
tiny one-class DOFA task (frozen encoder, batch 2, 3x32x32) with SoftBCEWithLogitsLoss(smooth_factor=0.1, ignore_index=255,
pos_weight) from a hipGraph -- one capture, three replays -- against an all-eager twin; prints one JSON line with the losses of
both and the number of ``upsample_logits`` calls (0: both heads' losses come from the low-resolution maps).  One scenario per
process (see tests/_graph_interleave_worker.py).  Stochastic layers are off and there is no global-norm clip (its float-atomic
reduction may move the last bit from run to run): everything else in the step, the soft-BCE kernels included, has a fixed
summation order."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "geo-deep-learning_amd", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import torch  # noqa: E402

import test_hip_binary_lowres as T  # noqa: E402
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402
from gdlhip.graphs import GraphedTrainStep  # noqa: E402


def make(capturable):
    task = T._one_class_dofa_task(gnn.SoftBCEWithLogitsLoss(smooth_factor=0.1, ignore_index=255, pos_weight=torch.tensor([1.5])))
    for blk in task.model.encoder.blocks:
        blk.drop_prob = 0.0
    task.model.aux_head.dropout_ratio = 0.0
    params = [p for p in task.parameters() if p.requires_grad]
    return task, gnn.FusedAdam(params, lr=1e-3, capturable=capturable)


def batch(seed):
    b = T._one_class_batch(seed, b=2)
    g = torch.Generator().manual_seed(seed)
    b["mask"][(torch.rand(b["mask"].shape, generator=g) < 0.2).to(b["mask"].device)] = 255
    return b


def main():
    calls = []
    real = ops.upsample_logits
    ops.upsample_logits = lambda *a, **k: calls.append(1) or real(*a, **k)
    batches = [batch(30 + i) for i in range(4)]
    te, oe = make(False)
    tg, og = make(True)
    graphed = GraphedTrainStep(tg, og, batches[0], autocast_dtype=None, warmup=2)
    te.train()
    for _ in range(2):      # the two warm-up steps were real optimizer steps on batches[0]
        oe.zero_grad(set_to_none=True)
        te.training_step(batches[0], 0).backward()
        oe.step()
    eager, replayed = [], []
    for b in batches[1:]:
        oe.zero_grad(set_to_none=True)
        le = te.training_step(b, 0)
        le.backward()
        oe.step()
        lg = graphed(b)
        torch.cuda.synchronize()
        eager.append(le.item().hex())
        replayed.append(lg.item().hex())
    print(json.dumps({"eager": eager, "graphed": replayed, "upsample_logits_calls": len(calls)}))


if __name__ == "__main__":
    main()
