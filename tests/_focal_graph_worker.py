"""Worker of tests/test_hip_focal.py::test_graphed_train_step_reproduces_the_eager_losses_bit_for_bit: training steps of the tiny
DOFA task (frozen encoder, batch 2, 3x112x112) with FocalLoss("multiclass", alpha=0.25) from a hipGraph -- one capture, two
replays -- against an all-eager twin; prints one JSON line with the losses of both.  One scenario per process (see
tests/_graph_interleave_worker.py).  Stochastic layers are off and there is no global-norm clip (its float-atomic reduction may
move the last bit from run to run): everything else in the step, the focal kernels included, has a fixed summation order."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "geo-deep-learning_amd", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import torch  # noqa: E402

import test_hip_soft_ce as S  # noqa: E402
from gdlhip import nn as gnn  # noqa: E402
from gdlhip.graphs import GraphedTrainStep  # noqa: E402


def make(capturable):
    task = S._dofa_task(gnn.FocalLoss("multiclass", alpha=0.25))
    for blk in task.model.encoder.blocks:
        blk.drop_prob = 0.0
    task.model.aux_head.dropout_ratio = 0.0
    params = [p for p in task.parameters() if p.requires_grad]
    return task, gnn.FusedAdam(params, lr=1e-3, capturable=capturable)


def main():
    batches = [S._dofa_batch(30 + i, b=2) for i in range(3)]
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
    print(json.dumps({"eager": eager, "graphed": replayed}))


if __name__ == "__main__":
    main()
