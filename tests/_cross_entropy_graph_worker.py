"""Worker of tests/test_hip_cross_entropy.py::test_graphed_train_step_reproduces_the_eager_losses_bit_for_bit: training steps of
the tiny DOFA task (frozen encoder, batch 2, 3x112x112) with a weighted mean CrossEntropyLoss(ignore_index=255) from a hipGraph
-- one capture, three replays -- against an all-eager twin; prints one JSON line with the losses of both.  Each batch ignores a
different fraction of its pixels (the capture batch none), so the mean's divisor, the summed class weights of the valid pixels,
differs from replay to replay: it has to be formed on the device inside the graph.  One scenario per process (see
tests/_graph_interleave_worker.py).  Stochastic layers are off and there is no global-norm clip (its float-atomic reduction may
move the last bit from run to run): everything else in the step, the cross-entropy kernels included, has a fixed summation order."""
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

WEIGHT = [0.25, 1.0, 0.0, 2.0, 1.5]
IGNORED = [0.0, 0.1, 0.35, 0.6]      # the capture batch, then the three replays


def make(capturable):
    task = S._dofa_task(gnn.CrossEntropyLoss(weight=torch.tensor(WEIGHT), ignore_index=255))
    for blk in task.model.encoder.blocks:
        blk.drop_prob = 0.0
    task.model.aux_head.dropout_ratio = 0.0
    params = [p for p in task.parameters() if p.requires_grad]
    return task, gnn.FusedAdam(params, lr=1e-3, capturable=capturable)


def batch(i):
    b = S._dofa_batch(30 + i, b=2)
    hide = torch.rand(b["mask"].shape, generator=torch.Generator().manual_seed(i)) < IGNORED[i]
    b["mask"][hide.to(b["mask"].device)] = 255
    return b


def main():
    batches = [batch(i) for i in range(len(IGNORED))]
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
    ignored = [int((b["mask"] == 255).sum().item()) for b in batches[1:]]
    print(json.dumps({"eager": eager, "graphed": replayed, "ignored": ignored}))


if __name__ == "__main__":
    main()
