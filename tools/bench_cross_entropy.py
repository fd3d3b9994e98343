#!/usr/bin/env python
"""The cross-entropy tail of one DOFA-base training step (both heads: 144^2 and 18^2 -> 512^2, batch 64, 5 classes, class weights,
20 % ignored pixels; forward + backward per head through autograd, the auxiliary head with its 0.4 upstream factor), us per step, for
  (a) materialised + torch       -- LowresLogits.materialise() + torch.nn.CrossEntropyLoss(weight=w): what a user had before,
  (b) materialised + HIP         -- LowresLogits.materialise() + gdlhip.nn.CrossEntropyLoss: gdl_cross_entropy_fwd / _bwd,
  (c) low-resolution             -- gdlhip.nn.CrossEntropyLoss on LowresLogits: gdl_cross_entropy_lowres_fwd / _bwd (tile form),
  (d) SoftCrossEntropyLoss       -- its low-resolution recompute form (gdl_soft_ce_lowres_fwd / _bwd), the yardstick.
The variants run in one process and alternate round by round; times are HIP events around ``--inner`` steps.  Every variant's loss
and d(low) are compared with (a)'s before anything is timed.  ``--out FILE`` also writes the report to FILE."""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "geo-deep-learning_amd"))
from gdlhip import nn as gnn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--out", type=Path, default=None)
args = ap.parse_args()

B, K, H = args.batch, 5, 512
HEADS = ((144, 1.0), (18, 0.4))
g = torch.Generator(device="cuda").manual_seed(0)
lows = [(torch.randn(B, h, h, K, device="cuda", generator=g) * 2).requires_grad_(True) for h, _ in HEADS]
tgt = torch.randint(0, K, (B, H, H), device="cuda", generator=g)
tgt[torch.rand(tgt.shape, device="cuda", generator=g) < 0.2] = 255
weight = torch.tensor([0.2, 1.0, 1.0, 2.0, 2.0], device="cuda")
torch_ce = torch.nn.CrossEntropyLoss(weight=weight, ignore_index=255)
hip_ce = gnn.CrossEntropyLoss(weight=weight, ignore_index=255)
soft_ce = gnn.SoftCrossEntropyLoss(ignore_index=255)
gnn.SOFT_CE_LOWRES_FUSED = False      # (d) is the recompute form: the new loss has no fused one


def tail(crit, materialise):
    """One step's loss tail: both heads' losses, one backward; returns the loss and the two d(low)."""
    for low in lows:
        low.grad = None
    total = 0.0
    for low, (_, up) in zip(lows, HEADS):
        logits = gnn.LowresLogits(low, (H, H))
        total = total + up * crit(logits.materialise() if materialise else logits, tgt)
    total.backward()
    return total.detach(), [low.grad for low in lows]


variants = {"(a) materialised + torch CE": lambda: tail(torch_ce, True), "(b) materialised + HIP CE": lambda: tail(hip_ce, True),
            "(c) low-resolution HIP CE": lambda: tail(hip_ce, False), "(d) SoftCE, low-res recompute": lambda: tail(soft_ce, False)}

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


ref_loss, ref_grads = variants["(a) materialised + torch CE"]()
for name in ("(b) materialised + HIP CE", "(c) low-resolution HIP CE"):
    loss, grads = variants[name]()
    err_l = abs(loss.item() - ref_loss.item()) / max(1.0, abs(ref_loss.item()))
    err_g = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(grads, ref_grads))
    assert err_l <= 2e-5 and err_g <= 1e-3, (name, err_l, err_g)      # against torch's own f32 kernels, not an f64 reference
    say(f"{name} vs (a): loss rel err {err_l:.2e}, d(low) max err {err_g:.2e} of its maximum")

for fn in variants.values():      # warm-up: every shape, every variant
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in variants}
for _ in range(args.rounds):           # the variants alternate round by round
    for name, fn in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) / args.inner * 1e3)

say(f"CrossEntropyLoss(weight, ignore_index=255) tail, both heads ({HEADS[0][0]}^2 and {HEADS[1][0]}^2 -> {H}^2), batch {B}, K = {K}; "
    f"us per step (forward + backward), {args.rounds} rounds of {args.inner} steps, variants alternating")
base = sorted(times["(a) materialised + torch CE"])[args.rounds // 2]
for name, ts in times.items():
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    say(f"  {name:32s} median {med:9.1f}  min {ts[0]:9.1f}  max {ts[-1]:9.1f}   ({med / base:5.3f} x (a))")
if args.out is not None:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")
