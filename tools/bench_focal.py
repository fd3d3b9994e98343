#!/usr/bin/env python
"""The FocalLoss tail of one DOFA-base training step (both heads: 144^2 and 18^2 -> 512^2, batch 64, 5 classes; forward + backward
per head, the auxiliary head with its 0.4 upstream factor), us per step, for
  (a) low-resolution, tile       -- gdl_focal_lowres_fwd (partial sums) / _bwd, form GDL_FOCAL_TILE (tile kernel + patch reduce),
  (b) low-resolution, gather     -- the same forward / _bwd, form GDL_FOCAL_GATHER,
  (c) materialised               -- gdl_upsample_logits + gdl_focal_fwd + gdl_focal_bwd + gdl_upsample_logits_bwd,
  (d) SoftCrossEntropyLoss       -- its default low-resolution form (fused) at the same shapes, the yardstick.
The variants run in one process and alternate round by round; times are HIP events around ``--inner`` steps.  Then the
full-resolution kernels alone (batch x 5 x 512^2): GB/s of algorithmic bytes (logits + targets read, gradient written)."""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "geo-deep-learning_amd"))
from gdlhip import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--inner", type=int, default=20)
args = ap.parse_args()

B, K, H = args.batch, 5, 512
HEADS = ((144, 1.0), (18, 0.4))
g = torch.Generator(device="cuda").manual_seed(0)
lows = [torch.randn(B, h, h, K, device="cuda", generator=g) * 2 for h, _ in HEADS]
tgt = torch.randint(0, K, (B, H, H), device="cuda", generator=g)
ups = [torch.tensor(w, device="cuda") for _, w in HEADS]
opt = ops.FocalOptions(2.0, 0.25, None, True, None)
ce_opt = ops.SoftCEOptions(0.1, -100, True)


def lowres_tail(form):
    out = []
    for low, up in zip(lows, ups):
        loss, norm = ops.focal_lowres_fwd(low, tgt, (H, H), opt)
        out.append((loss, ops.focal_lowres_bwd(low, tgt, (H, H), norm, up, 1.0, opt, form=form)))
    return out


def materialised_tail():
    out = []
    for low, up in zip(lows, ups):
        logits = ops.upsample_logits(low, (H, H))
        loss, norm = ops.focal_fwd(logits, tgt, opt)
        dlogits = ops.focal_bwd(logits, tgt, norm, up, 1.0, opt)
        out.append((loss, ops.upsample_logits_bwd(dlogits, (low.shape[1], low.shape[2]))))
    return out


def soft_ce_tail():
    out = []
    for low, up in zip(lows, ups):
        loss, state = ops.soft_ce_lowres_fwd(low, tgt, (H, H), ce_opt, fused=True)
        out.append((loss, ops.soft_ce_lowres_bwd(low, tgt, (H, H), up, 1.0, ce_opt, state=state)))
    return out


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


variants = {"(a) low-resolution, tile": lambda: lowres_tail("tile"), "(b) low-resolution, gather": lambda: lowres_tail("gather"),
            "(c) materialised": materialised_tail, "(d) SoftCrossEntropyLoss, fused": soft_ce_tail}
times = timed(variants, args.rounds, args.inner)
print(f"FocalLoss(multiclass, alpha=0.25, gamma=2) tail, both heads ({HEADS[0][0]}^2 and {HEADS[1][0]}^2 -> {H}^2), batch {B}, K = {K}; "
      f"us per step, {args.rounds} rounds of {args.inner} steps")
base = times["(c) materialised"][args.rounds // 2]
for name, ts in times.items():
    med = ts[len(ts) // 2]
    print(f"  {name:34s} median {med:8.1f}  min {ts[0]:8.1f}  max {ts[-1]:8.1f}   ({med / base:5.3f} x materialised)")
ref = materialised_tail()
for name, fn in list(variants.items())[:2]:
    for (la, ga), (lb, gb) in zip(fn(), ref):
        err_l = abs(la.item() - lb.item()) / max(1.0, abs(lb.item()))
        err_g = (ga - gb).abs().max().item() / gb.abs().max().item()
        assert err_l <= 2e-6 and err_g <= 1e-4, (name, err_l, err_g)
print("low-resolution forms agree with the materialised path (loss 2e-6, gradient 1e-4 of its maximum)")

logits = ops.upsample_logits(lows[0], (H, H))
dl = torch.empty_like(logits)
_, norm0 = ops.focal_fwd(logits, tgt, opt)
full = timed({"fwd": lambda: ops.focal_fwd(logits, tgt, opt), "bwd": lambda: ops.focal_bwd(logits, tgt, norm0, ups[0], 1.0, opt, out=dl)},
             args.rounds, args.inner)
read = logits.numel() * 4 + tgt.numel() * 8
for name, nbytes in (("fwd", read), ("bwd", read + logits.numel() * 4)):
    med = full[name][args.rounds // 2]
    print(f"full resolution {name} [{B}, {K}, {H}, {H}]: median {med:8.1f} us  {nbytes / med * 1e-3:7.1f} GB/s of {nbytes / 1e6:.0f} MB "
          f"(min {full[name][0]:.1f} us, max {full[name][-1]:.1f} us)")
