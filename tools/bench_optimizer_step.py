#!/usr/bin/env python
"""What the fused AdamW / SGD buy, measured two ways.

(1) clip + update alone: the trainable parameters of DOFA-base + UperNet (encoder frozen, and everything trainable), random
    gradients written in place, max_grad_norm 1.0 -- ``clip_grad_norm_`` + ``torch.optim.AdamW`` / ``SGD`` (foreach) against
    ``gdlhip.nn.FusedAdamW`` / ``FusedSGD``.  HIP events around ONE clip + update, warm, the variants alternating rep by rep;
    median / min / max in us.  No bf16 operands exist here, so the shadow and repack work of a bf16 training step is not in it.
(2) ``MiniTrainer.fit`` train tiles/s at per-GPU batch 4, 512x512, bf16, ``torch.optim.AdamW`` from configure_optimizers:
    ``use_fused_adam=False`` (torch's AdamW + clip_grad_norm_, eager step: what the trainer did with AdamW before the fused
    class existed) against the default (FusedAdamW, step captured into a hipGraph).  One child process per run, the two
    alternating; the first epoch (warm-up, capture) is not timed.

    python tools/bench_optimizer_step.py [--reps 30] [--rounds 3] [--skip-step | --skip-trainer]"""
import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from functools import partial
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "geo-deep-learning_amd")]
from gdlhip import nn as gnn  # noqa: E402

DEV = torch.device("cuda", 0)


def dofa_task(freeze, optimizer, size=512):
    from geo_deep_learning.tasks_with_models.segmentation_dofa import SegmentationDOFA
    task = SegmentationDOFA(encoder="dofa_base", pretrained=False, image_size=(size, size), num_classes=5, max_samples=6,
                            loss=gnn.DiceLoss(mode="multiclass"), freeze_layers=["encoder"] if freeze else None,
                            wavelengths=[0.665, 0.549, 0.481], optimizer=optimizer,
                            scheduler=partial(torch.optim.lr_scheduler.StepLR, step_size=1000), scheduler_config={"interval": "epoch"})
    task.configure_model()
    return task.to(DEV)


# ------------------------------------------------------------------------------------------------ (1) clip + update
def step_times(reps):
    cases = {"AdamW": (torch.optim.AdamW, gnn.FusedAdamW, dict(lr=1e-3, weight_decay=1e-2)),
             "SGD momentum 0.9": (torch.optim.SGD, gnn.FusedSGD, dict(lr=0.05, momentum=0.9)),
             "SGD plain": (torch.optim.SGD, gnn.FusedSGD, dict(lr=0.05))}
    for freeze in (True, False):
        task = dofa_task(freeze, partial(torch.optim.AdamW, lr=1e-3))
        shapes = [p.detach() for p in task.parameters() if p.requires_grad]
        n = sum(p.numel() for p in shapes)
        print(f"DOFA-base + UperNet, encoder {'frozen' if freeze else 'trainable'}: {len(shapes)} tensors, {n / 1e6:.1f} M parameters; "
              f"clip + update, us, median (min .. max) of {reps}")
        for name, (torch_cls, fused_cls, kw) in cases.items():
            sides = {}
            for side, make in (("torch foreach", lambda ps: torch_cls(ps, foreach=True, **kw)),              # noqa: B023
                               ("fused", lambda ps: fused_cls(ps, max_grad_norm=1.0, **kw)),                   # noqa: B023
                               ("fused capturable", lambda ps: fused_cls(ps, max_grad_norm=1.0, capturable=True, **kw))):   # noqa: B023
                ps = [p.clone().requires_grad_(True) for p in shapes]
                for p in ps:
                    p.grad = torch.randn_like(p)
                sides[side] = (ps, make(ps))

            def run(side):
                ps, opt = sides[side]                                                                             # noqa: B023
                if side == "torch foreach":
                    torch.nn.utils.clip_grad_norm_(ps, 1.0)
                opt.step()

            for side in sides:
                for _ in range(3):
                    run(side)
            torch.cuda.synchronize()
            times = {side: [] for side in sides}
            for _ in range(reps):
                for side in sides:
                    for p in sides[side][0][:1]:
                        p.grad.normal_()           # (clip_grad_norm_ scaled the gradients in place: keep the norm above 1)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(side)
                    e1.record()
                    torch.cuda.synchronize()
                    times[side].append(e0.elapsed_time(e1) * 1e3)
            for side, ts in times.items():
                print(f"  {name:18s} {side:18s} {statistics.median(ts):9.1f}  ({min(ts):.1f} .. {max(ts):.1f})")
        del task


# ------------------------------------------------------------------------------------------------ (2) MiniTrainer
def trainer_child(fused, batches_per_epoch, epochs):
    import oracle
    from gdlhip.trainer import MiniTrainer, seed_everything
    seed_everything(42)
    task = dofa_task(True, partial(torch.optim.AdamW, lr=6e-5))
    base = [oracle.synthetic_batch(4, 3, 512, 5, s) for s in range(4)]
    for b in base:
        b["mask"] = b["mask"].long()
    batches = [base[i % len(base)] for i in range(batches_per_epoch)]
    marks = []

    original = getattr(task, "on_train_epoch_end", None)

    def epoch_end():
        if original is not None:
            original()
        torch.cuda.synchronize()
        marks.append(time.perf_counter())

    task.on_train_epoch_end = epoch_end
    tr = MiniTrainer(max_epochs=epochs, precision="bf16-mixed", gradient_clip_val=1.0, default_root_dir=tempfile.mkdtemp(),
                     use_fused_adam=fused)
    tr.fit(task, train_dataloaders=batches, val_dataloaders=None)
    per_epoch = [b - a for a, b in zip(marks, marks[1:])]          # the first epoch (warm-up, capture) only sets the first mark
    print(json.dumps({"optimizer": type(tr._optimizers[0]).__name__, "graphed_steps": tr.graphed_steps, "steps": tr.global_step,
                      "tiles_per_s": [round(4 * batches_per_epoch / t, 1) for t in per_epoch]}))


def trainer_runs(rounds, batches_per_epoch, epochs):
    results = {"torch AdamW, eager": [], "FusedAdamW, captured": []}
    for _ in range(rounds):
        for name, flag in (("torch AdamW, eager", "0"), ("FusedAdamW, captured", "1")):
            run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, __file__, "--child", flag, "--batches", str(batches_per_epoch),
                                  "--epochs", str(epochs)], capture_output=True, text=True)
            if run.returncode != 0:
                print(f"{name}: child ended with status {run.returncode}; stopping\n{run.stdout[-2000:]}{run.stderr[-3000:]}")
                sys.exit(1)
            res = json.loads(run.stdout.strip().splitlines()[-1])
            print(f"  {name}: {res}")
            results[name] += res["tiles_per_s"]
    print(f"MiniTrainer.fit, DOFA-base + UperNet (encoder frozen), per-GPU batch 4, bf16, AdamW + clip 1.0; train tiles/s per epoch of "
          f"{batches_per_epoch} batches (host batches, H2D and augmentation included)")
    for name, v in results.items():
        print(f"  {name:24s} median {statistics.median(v):7.1f}  min {min(v):7.1f}  max {max(v):7.1f}  ({len(v)} epochs)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.child is not None:
        trainer_child(args.child == "1", args.batches, args.epochs)
        sys.exit(0)
    if not args.skip_step:
        step_times(max(20, args.reps))
    if not args.skip_trainer:
        trainer_runs(args.rounds, args.batches, args.epochs)
