#!/usr/bin/env python
"""The one-class (binary) step tail of a DOFA-base model, per head shape, at batch 64: the main head 128^2 -> 512^2 and the
auxiliary head 16^2 -> 512^2 with its 0.4 upstream factor; 64^2 and 32^2 in between locate the factor at which the routes
cross.  us per call from HIP events around ``--inner`` calls, the variants alternating round by round in one process.
Loss forward + backward, for binary DiceLoss and binary FocalLoss(alpha=0.25, gamma=2):
  (a) low-resolution, tile    -- gdl_*_binary_*lowres_fwd (partial sums) / _bwd in the tile form (tile kernel + patch reduce),
  (b) low-resolution, gather  -- the same forward / _bwd in the gather form,
  (c) materialised            -- what a one-class step ran before: gdl_upsample_logits + the full-resolution binary loss
                                 forward and backward + gdl_upsample_logits_bwd.
The mask of validation / test:
  (d) gdl_upsample_threshold                                      -- from the low-resolution map,
  (e) gdl_upsample_logits + gdl_sigmoid_threshold                 -- resized logits, one pass,
  (f) gdl_upsample_logits + (x.sigmoid().squeeze(1) > th).long()  -- resized logits, the three torch ops of the earlier _predict.
Every low-resolution result is checked against the materialised one before it is timed.  The committed output is
profiles/bench_binary_lowres.txt."""
import argparse
import sys
from pathlib import Path

import torch

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
print(f"tools/bench_binary_lowres.py --batch {args.batch} --rounds {args.rounds} --inner {args.inner} --sizes {args.sizes}   "
      f"({torch.cuda.get_device_name(0)}, torch {torch.__version__})")
NAMES = {128: ("main head", 1.0), 16: ("auxiliary head", 0.4)}      # the other sizes locate the factor where the routes cross
HEADS = tuple((*NAMES.get(int(h), (f"factor {512 // int(h)}", 1.0)), int(h)) for h in args.sizes.split(","))
g = torch.Generator(device="cuda").manual_seed(0)
tgt = torch.randint(0, 2, (B, H, H), device="cuda", generator=g)
fopt = ops.FocalOptions(2.0, 0.25, None, True, None)


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
        print(f"  {name:58s} median {med:8.1f}  min {ts[0]:8.1f}  max {ts[-1]:8.1f}   ({med / ref:5.3f} x {base[:3]})")


def agree(name, got, ref):
    (la, ga), (lb, gb) = got, ref
    err_l = abs(la.item() - lb.item()) / max(1.0, abs(lb.item()))
    err_g = (ga - gb).abs().max().item() / gb.abs().max().item()
    assert err_l <= 2e-6 and err_g <= 1e-4, (name, err_l, err_g)


for head, w, h in HEADS:
    low = torch.randn(B, h, h, 1, device="cuda", generator=g) * 2
    up = torch.tensor(w, device="cuda")

    def dice_lowres(form):
        loss, sums = ops.dice_binary_lowres_fwd(low, tgt, (H, H))
        return loss, ops.dice_binary_lowres_bwd(low, tgt, (H, H), sums, up, form=form)

    def dice_materialised():
        logits = ops.upsample_logits(low, (H, H))
        loss, sums = ops.dice_binary_loss_fwd(logits, tgt)
        return loss, ops.upsample_logits_bwd(ops.dice_binary_loss_bwd(logits, tgt, sums, up), (h, h))

    def focal_lowres(form):
        loss, norm = ops.focal_binary_lowres_fwd(low, tgt, (H, H), fopt)
        return loss, ops.focal_binary_lowres_bwd(low, tgt, (H, H), norm, up, 1.0, fopt, form=form)

    def focal_materialised():
        logits = ops.upsample_logits(low, (H, H))
        loss, norm = ops.focal_binary_fwd(logits, tgt, fopt)
        return loss, ops.upsample_logits_bwd(ops.focal_binary_bwd(logits, tgt, norm, up, 1.0, fopt), (h, h))

    for loss_name, lowres, materialised in (("DiceLoss(binary)", dice_lowres, dice_materialised),
                                            ("FocalLoss(binary, alpha=0.25, gamma=2)", focal_lowres, focal_materialised)):
        for form in ("tile", "gather"):
            agree((head, loss_name, form), lowres(form), materialised())
        variants = {"(a) low-resolution, tile": lambda: lowres("tile"), "(b) low-resolution, gather": lambda: lowres("gather"),
                    "(c) materialised": materialised}
        report(f"{loss_name} forward + backward, {head} {h}^2 -> {H}^2, batch {B}; us per call, {args.rounds} rounds of {args.inner}",
               timed(variants, args.rounds, args.inner), "(c) materialised")

    th = 0.5
    want = ops.sigmoid_threshold(ops.upsample_logits(low, (H, H)), th)
    assert torch.equal(ops.upsample_threshold(low, (H, H), th), want)
    torch_ops = (ops.upsample_logits(low, (H, H)).sigmoid().squeeze(1) > th).long()
    print(f"mask: {(torch_ops != want).sum().item()} of {want.numel()} pixels differ between the kernels and the torch expression")
    variants = {"(d) upsample_threshold": lambda: ops.upsample_threshold(low, (H, H), th),
                "(e) upsample_logits + sigmoid_threshold": lambda: ops.sigmoid_threshold(ops.upsample_logits(low, (H, H)), th),
                "(f) upsample_logits + (x.sigmoid().squeeze(1) > th).long()": lambda: (ops.upsample_logits(low, (H, H)).sigmoid().squeeze(1) > th).long()}
    report(f"mask, {head} {h}^2 -> {H}^2, batch {B}; us per call", timed(variants, args.rounds, args.inner),
           "(f) upsample_logits + (x.sigmoid().squeeze(1) > th).long()")
print("low-resolution forms agree with the materialised path (loss 2e-6, gradient 1e-4 of its maximum; masks equal)")
