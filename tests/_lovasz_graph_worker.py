"""Worker of tests/test_hip_lovasz.py::test_graphed_train_step_reproduces_the_eager_losses_bit_for_bit: training steps of the toy
task (tests/_toy_task.py, batch 8, 3x8x8, 3 classes) with LovaszLoss("multiclass", ignore_index=255) from a hipGraph -- one capture,
three replays -- against an all-eager twin; prints one JSON line with the losses of both.  One scenario per process (see
tests/_graph_interleave_worker.py).  The sort's passes, the count scan and the loss sum have a fixed launch sequence and summation
order and nothing in them reads back to the host, so the step records and replays to the same bits."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "geo-deep-learning_amd", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import torch  # noqa: E402

import _toy_task as toy  # noqa: E402
from gdlhip import nn as gnn  # noqa: E402
from gdlhip.graphs import GraphedTrainStep  # noqa: E402


def make(capturable):
    torch.manual_seed(11)
    task = toy.ToyTask(3, gnn.LovaszLoss("multiclass", ignore_index=255))
    task.configure_model()
    task = task.cuda()
    return task, gnn.FusedAdam(list(task.parameters()), lr=1e-2, capturable=capturable)


def main():
    batches = [{k: v.cuda() for k, v in b.items()} for b in toy.make_batches(4, 8, 3, 5)]
    for b in batches:
        b["mask"][:, :, 0] = 255      # a row of ignored pixels
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
