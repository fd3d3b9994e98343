"""Worker of the five ``test_graphed_*_reproduces_the_eager_losses_bit_for_bit`` tests (tests/test_hip_focal.py,
test_hip_lovasz.py, test_hip_binary_lowres.py, test_hip_soft_bce.py, test_hip_cross_entropy.py): training steps of a tiny task
with one loss from a hipGraph -- one capture, then one replay per further batch -- against an all-eager twin; prints one JSON line
with the losses of both (as hex) and the scenario's own keys.  The scenario is the first argument; one scenario per process (see
tests/_graph_interleave_worker.py).  Stochastic layers are off and there is no global-norm clip (its float-atomic reduction may
move the last bit from run to run): everything else in a step, the loss kernels included, has a fixed launch sequence and
summation order and reads nothing back to the host, so the step records and replays to the same bits."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "geo-deep-learning_amd", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import torch  # noqa: E402

from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402
from gdlhip.graphs import GraphedTrainStep  # noqa: E402

XENT_WEIGHT = [0.25, 1.0, 0.0, 2.0, 1.5]
XENT_IGNORED = [0.0, 0.1, 0.35, 0.6]      # the capture batch, then the three replays


def _dofa(task):
    """(task, the parameters it trains, lr) of a tiny DOFA task (frozen encoder) with its stochastic layers off."""
    for blk in task.model.encoder.blocks:
        blk.drop_prob = 0.0
    task.model.aux_head.dropout_ratio = 0.0
    return task, [p for p in task.parameters() if p.requires_grad], 1e-3


def _hide(batch, fraction, seed):
    """``batch`` with that fraction of its mask set to 255 (the scenarios' ignore_index)."""
    hide = torch.rand(batch["mask"].shape, generator=torch.Generator().manual_seed(seed)) < fraction
    batch["mask"][hide.to(batch["mask"].device)] = 255
    return batch


# A scenario returns (make, batches, extra): ``make()`` builds a fresh (task, parameters, lr); ``batches[0]`` is the capture and
# warm-up batch, every further one is one replay; ``extra(batches, upsample_logits_calls)`` is what the JSON line holds besides
# the losses.
def focal():
    """FocalLoss("multiclass", alpha=0.25) from the low-resolution logits of the tiny DOFA task (batch 2, 3x112x112); two replays."""
    import test_hip_soft_ce as S
    return (lambda: _dofa(S._dofa_task(gnn.FocalLoss("multiclass", alpha=0.25))), [S._dofa_batch(30 + i, b=2) for i in range(3)],
            lambda batches, calls: {})


def cross_entropy():
    """A weighted mean CrossEntropyLoss(ignore_index=255) on the same task; three replays.  Each batch ignores a different
    fraction of its pixels (the capture batch none), so the mean's divisor, the summed class weights of the valid pixels, differs
    from replay to replay: it has to be formed on the device inside the graph."""
    import test_hip_soft_ce as S
    batches = [_hide(S._dofa_batch(30 + i, b=2), XENT_IGNORED[i], i) for i in range(len(XENT_IGNORED))]
    return (lambda: _dofa(S._dofa_task(gnn.CrossEntropyLoss(weight=torch.tensor(XENT_WEIGHT), ignore_index=255))), batches,
            lambda batches, calls: {"ignored": [int((b["mask"] == 255).sum().item()) for b in batches[1:]]})


def binary_lowres():
    """DiceLoss(mode="binary") on the tiny one-class DOFA task (batch 2, 3x32x32); two replays.  ``upsample_logits_calls`` 0: both
    heads' losses come from the low-resolution maps."""
    import test_hip_binary_lowres as T
    return (lambda: _dofa(T._one_class_dofa_task(gnn.DiceLoss(mode="binary"))), [T._one_class_batch(30 + i, b=2) for i in range(3)],
            lambda batches, calls: {"upsample_logits_calls": calls})


def soft_bce():
    """SoftBCEWithLogitsLoss(smooth_factor=0.1, ignore_index=255, pos_weight) on the one-class task, a fifth of every mask
    ignored; three replays; ``upsample_logits_calls`` as binary_lowres."""
    import test_hip_binary_lowres as T
    crit = lambda: gnn.SoftBCEWithLogitsLoss(smooth_factor=0.1, ignore_index=255, pos_weight=torch.tensor([1.5]))  # noqa: E731
    return (lambda: _dofa(T._one_class_dofa_task(crit())), [_hide(T._one_class_batch(30 + i, b=2), 0.2, 30 + i) for i in range(4)],
            lambda batches, calls: {"upsample_logits_calls": calls})


def lovasz():
    """LovaszLoss("multiclass", ignore_index=255) on the toy task (tests/_toy_task.py, batch 8, 3x8x8, 3 classes), a row of every
    mask ignored; three replays."""
    import _toy_task as toy

    def make():
        torch.manual_seed(11)
        task = toy.ToyTask(3, gnn.LovaszLoss("multiclass", ignore_index=255))
        task.configure_model()
        task = task.cuda()
        return task, list(task.parameters()), 1e-2

    batches = [{k: v.cuda() for k, v in b.items()} for b in toy.make_batches(4, 8, 3, 5)]
    for b in batches:
        b["mask"][:, :, 0] = 255
    return make, batches, lambda batches, calls: {}


SCENARIOS = {f.__name__: f for f in (focal, cross_entropy, binary_lowres, soft_bce, lovasz)}


def main(scenario):
    calls = []
    real = ops.upsample_logits
    ops.upsample_logits = lambda *a, **k: calls.append(1) or real(*a, **k)
    make, batches, extra = SCENARIOS[scenario]()

    def optimizer(capturable):
        task, params, lr = make()
        return task, gnn.FusedAdam(params, lr=lr, capturable=capturable)

    te, oe = optimizer(False)
    tg, og = optimizer(True)
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
    print(json.dumps({"eager": eager, "graphed": replayed, **extra(batches, len(calls))}))


if __name__ == "__main__":
    main(sys.argv[1])
