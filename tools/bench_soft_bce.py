#!/usr/bin/env python
"""SoftBCEWithLogitsLoss(smooth_factor=0.1, ignore_index=255) forward + backward for a one-class DOFA-base model, per head shape,
at batch 64 in f32: the main head 128^2 -> 512^2 and the auxiliary head 16^2 -> 512^2 with its 0.4 upstream factor; ``--sizes``
adds sizes in between to locate the factor at which the routes cross.  us per call from HIP events around ``--inner`` calls, the
variants alternating round by round in one process, for an int64 and an f32 target:
  (a) low-resolution, tile    -- gdl_soft_bce_lowres_fwd (partial sums) / _bwd in the tile form (tile kernel + patch reduce),
  (b) low-resolution, gather  -- the same forward / _bwd in the gather form,
  (c) materialised            -- the class's own other route: gdl_upsample_logits + gdl_soft_bce_fwd / _bwd +
                                 gdl_upsample_logits_bwd,
  (d) torch                   -- gdl_upsample_logits + smp's forward on torch ops (the smoothed target, F.binary_cross_entropy_with_logits,
                                 the ignore mask, mean) and torch.autograd.grad + gdl_upsample_logits_bwd.
Every low-resolution result is checked against the materialised one before it is timed.  The committed output is
profiles/bench_soft_bce.txt."""
import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "geo-deep-learning_amd"))
from gdlhip import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--sizes", default="128,64,32,16", help="low-resolution sizes h (h^2 -> 512^2); DOFA's heads are 128 and 16")
args = ap.parse_args()

B, H = args.batch, 512
print(f"tools/bench_soft_bce.py --batch {args.batch} --rounds {args.rounds} --inner {args.inner} --sizes {args.sizes}   "
      f"({torch.cuda.get_device_name(0)}, torch {torch.__version__})")
NAMES = {128: ("main head", 1.0), 16: ("auxiliary head", 0.4)}      # the other sizes locate the factor where the routes cross
HEADS = tuple((*NAMES.get(int(h), (f"factor {512 // int(h)}", 1.0)), int(h)) for h in args.sizes.split(","))
SMOOTH, IGNORE = 0.1, 255
g = torch.Generator(device="cuda").manual_seed(0)
tgt_i = torch.randint(0, 2, (B, H, H), device="cuda", generator=g)
tgt_i[torch.rand((B, H, H), device="cuda", generator=g) < 0.1] = IGNORE
TARGETS = {"int64": tgt_i, "f32": tgt_i.float()}
opt = ops.SoftBCEOptions(SMOOTH, IGNORE, True, None, None)


def timed(variants, rounds, inner):
    for fn in variants.values():      # warm-up: every shape, every variant
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):           # the variants alternate round by round
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner * 1e3)
    return {k: sorted(v) for k, v in times.items()}


def report(title, times, base):
    print(title)
    ref = times[base][len(times[base]) // 2]
    for name, ts in times.items():
        med = ts[len(ts) // 2]
        print(f"  {name:32s} median {med:8.1f}  min {ts[0]:8.1f}  max {ts[-1]:8.1f}   ({med / ref:5.3f} x {base[:3]})")


def agree(name, got, ref):
    (la, ga), (lb, gb) = got, ref
    err_l = abs(la.item() - lb.item()) / max(1.0, abs(lb.item()))
    err_g = (ga - gb).abs().max().item() / gb.abs().max().item()
    assert err_l <= 2e-6 and err_g <= 1e-4, (name, err_l, err_g)


for head, w, h in HEADS:
    low = torch.randn(B, h, h, 1, device="cuda", generator=g) * 2
    up = torch.tensor(w, device="cuda")
    for tname, tgt in TARGETS.items():
        def lowres(form):
            loss = ops.soft_bce_lowres_fwd(low, tgt, (H, H), opt)
            return loss, ops.soft_bce_lowres_bwd(low, tgt, (H, H), up, 1.0, opt, form=form)

        def materialised():
            logits = ops.upsample_logits(low, (H, H))
            loss = ops.soft_bce_fwd(logits, tgt, opt)
            return loss, ops.upsample_logits_bwd(ops.soft_bce_bwd(logits, tgt, up, 1.0, opt), (h, h))

        def torch_ops():
            logits = ops.upsample_logits(low, (H, H)).requires_grad_(True)
            y = tgt[:, None]
            soft = (1 - y) * SMOOTH + y * (1 - SMOOTH)
            loss = (F.binary_cross_entropy_with_logits(logits, soft, reduction="none") * (y != IGNORE)).mean()
            (grad,) = torch.autograd.grad(loss, logits, up)
            return loss.detach(), ops.upsample_logits_bwd(grad, (h, h))

        for form in ("tile", "gather"):
            agree((head, tname, form), lowres(form), materialised())
        agree((head, tname, "torch"), torch_ops(), materialised())
        variants = {"(a) low-resolution, tile": lambda: lowres("tile"), "(b) low-resolution, gather": lambda: lowres("gather"),
                    "(c) materialised": materialised, "(d) torch": torch_ops}
        report(f"SoftBCEWithLogitsLoss forward + backward, {tname} target, {head} {h}^2 -> {H}^2, batch {B}; us per call, "
               f"{args.rounds} rounds of {args.inner}", timed(variants, args.rounds, args.inner), "(c) materialised")
print("the low-resolution forms and the torch expression agree with the materialised route (loss 2e-6, gradient 1e-4 of its maximum)")
