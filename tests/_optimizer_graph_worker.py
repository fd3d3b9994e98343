"""Worker of tests/test_hip_optimizers.py::test_captured_step_equals_the_eager_twin: training steps of the tiny DOFA task (frozen
encoder, batch 2, 3x112x112) from a hipGraph with FusedAdamW / FusedSGD(capturable=True), one eager step in between, against an
all-eager twin with the host-argument form of the same optimizer; prints one JSON line.  ``argv``: adamw|sgd  f32|bf16.
One scenario per process (see tests/_graph_interleave_worker.py).  No global-norm clip: its float-atomic reduction may move the
last bit of the clip coefficient from run to run, and the losses are compared bit for bit."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "geo-deep-learning_amd", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import torch  # noqa: E402

import test_hip_tasks as T  # noqa: E402
from gdlhip import nn as gnn  # noqa: E402
from gdlhip.graphs import GraphedTrainStep  # noqa: E402


def make(kind, capturable):
    _, task = T._dofa_task(freeze=("encoder",))
    task.trainer = T._Trainer(True)
    for blk in task.model.encoder.blocks:
        blk.drop_prob = 0.0
    task.model.aux_head.dropout_ratio = 0.0
    params = [p for p in task.parameters() if p.requires_grad]
    if kind == "adamw":
        return task, gnn.FusedAdamW(params, lr=1e-3, weight_decay=1e-2, capturable=capturable)
    return task, gnn.FusedSGD(params, lr=0.01, momentum=0.9, capturable=capturable)


def eager_step(task, opt, b, amp):
    task.train()
    opt.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp is not None):
        loss = task.training_step(b, 0)
    loss.backward()
    opt.step()
    return loss


def main():
    kind, precision = sys.argv[1], sys.argv[2]
    amp = torch.bfloat16 if precision == "bf16" else None
    torch.manual_seed(1234)
    batches = [T._to_dev(T.synthetic_batch(2, 3, 112, 5, 50 + i)) for i in range(5)]
    for b in batches:
        b["mask"] = b["mask"].long()
    te, oe = make(kind, False)
    tg, og = make(kind, True)
    graphed = GraphedTrainStep(tg, og, batches[0], autocast_dtype=amp, warmup=2)
    cared = 0 if og._repack is None else int(og._repack[1].shape[0])
    for _ in range(2):                                                  # the capture's two warm-up steps were real steps
        eager_step(te, oe, batches[0], amp)
    eager, mixed, replays, between = [], [], 0, 0
    for i, b in enumerate(batches):
        eager.append(eager_step(te, oe, b, amp).item())
        if i == 2:
            mixed.append(eager_step(tg, og, b, amp).item())
            between += 1
        else:
            mixed.append(graphed(b).item())
            replays += 1
    checked = wrong = 0
    for p in tg.parameters():
        for key, val, mode, c0, c1 in gnn.derived_operands(p):
            hit = gnn._CACHE[key]
            if hit[0] != ((p._version, gnn._RAW_WRITES.get(id(p), 0), p.data_ptr()),):
                continue                                                # (stale entries are rebuilt on use)
            m = p.detach().permute(0, 2, 3, 1).reshape(p.shape[0], -1, p.shape[1])
            if mode == gnn.REPACK_SLICE:
                want = m[:, :, c0:c1].reshape(p.shape[0], -1)
            elif mode == gnn.REPACK_TAPS:
                want = m[:, :, c0:c1].permute(1, 0, 2).reshape(-1, c1 - c0)
            else:
                want = p.detach().permute(1, 2, 3, 0).flip(1, 2).reshape(p.shape[1], -1)
            checked += 1
            wrong += int(not torch.equal(val, want.to(torch.bfloat16)))
    twin_step = {oe.state[p]["step"] for p in oe.state}
    print(json.dumps({"operands_under_the_optimizers_care": cared, "replays": replays, "eager_steps_in_between": between,
                      "losses_eager": [float.hex(v) for v in eager], "losses_graphed": [float.hex(v) for v in mixed],
                      "derived_operands_checked": checked, "derived_operands_wrong": wrong, "device_step": float(og.device_state(0)[0]),
                      "eager_twin_step": twin_step.pop() if len(twin_step) == 1 else sorted(twin_step)}))


if __name__ == "__main__":
    main()
