#!/usr/bin/env python
"""LovaszLoss("multiclass") forward + backward on full-resolution logits [batch, 5, 512, 512], us per call, for
  (a) gdl_lovasz_fwd + gdl_lovasz_bwd, one segment of batch x 512^2 per class (per_image=False),
  (b) the same with per_image=True (one segment of 512^2 per image and class),
  (c) the torch restatement of the same definition on the same GPU (softmax, torch.sort(stable, descending) through ATen,
      cumsum of the sorted label bits, autograd backward), per_image=False -- what a config would run without the kernels.
The variants run in one process and alternate round by round; times are HIP events around ``--inner`` calls.  Then the sort alone
(gdl_sort_desc_f32 against torch.sort on [5, batch x 512^2] keys) with its algorithmic bytes: per radix pass 4 B/key read by the
histogram, 8 B/key read and 8 B/key written by the scatter, 4 passes."""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "geo-deep-learning_amd"))
from gdlhip import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--inner", type=int, default=3)
args = ap.parse_args()

B, K, H = args.batch, 5, 512
g = torch.Generator(device="cuda").manual_seed(0)
logits = torch.randn(B, K, H, H, device="cuda", generator=g) * 2
tgt = torch.randint(0, K, (B, H, H), device="cuda", generator=g)
up = torch.tensor(1.0, device="cuda")
dl = torch.empty_like(logits)


def hip_step(per_image):
    opt = ops.LovaszOptions(per_image, None)
    loss, coef, norm = ops.lovasz_fwd(logits, tgt, opt)
    return loss, ops.lovasz_bwd(logits, tgt, coef, norm, up, 1.0, opt, out=dl)


def torch_step():
    x = logits.detach().requires_grad_(True)
    p = torch.softmax(x, 1).permute(1, 0, 2, 3).reshape(K, -1)
    z = tgt.reshape(1, -1) == torch.arange(K, device="cuda")[:, None]
    e = (z.float() - p).abs()
    es, perm = torch.sort(e, dim=1, descending=True, stable=True)
    zs = torch.gather(z, 1, perm).long()
    G, P = zs.sum(1, keepdim=True), zs.cumsum(1)
    U = G + torch.arange(1, zs.shape[1] + 1, device="cuda") - P
    coef = torch.where(zs == 1, 1.0 / U.double(), (G - P).double() / ((U - 1) * U).clamp(min=1).double()).float()
    present = (G[:, 0] > 0).float()
    loss = ((es * coef).sum(1) * present).sum() / present.sum().clamp(min=1.0)
    loss.backward()
    return loss.detach(), x.grad


def timed(variants, rounds, inner):
    for fn in variants.values():      # warm-up: every shape, every variant
        for _ in range(2):
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


variants = {"(a) HIP, per_image=False": lambda: hip_step(False), "(b) HIP, per_image=True": lambda: hip_step(True),
            "(c) torch restatement (ATen sort)": torch_step}
times = timed(variants, args.rounds, args.inner)
print(f"LovaszLoss(multiclass) forward + backward, logits [{B}, {K}, {H}, {H}]; us per call, {args.rounds} rounds of {args.inner} calls")
base = times["(c) torch restatement (ATen sort)"][args.rounds // 2]
for name, ts in times.items():
    med = ts[len(ts) // 2]
    print(f"  {name:36s} median {med:10.1f}  min {ts[0]:10.1f}  max {ts[-1]:10.1f}   ({med / base:5.3f} x torch)")
(la, ga), (lc, gc) = hip_step(False), torch_step()
err_l, err_g = abs(la.item() - lc.item()), ((ga - gc).abs().max() / gc.abs().max()).item()
# (the restatement adds batch x 512^2 f32 terms per class in f32: at batch 64 its sum carries about 1e-5; the kernels' f64 partials do not)
print(f"HIP vs torch restatement: loss {la.item():.8f} vs {lc.item():.8f} (diff {err_l:.2e}), gradient diff {err_g:.2e} of its maximum")
assert err_l <= 5e-5 and err_g <= 1e-2, (err_l, err_g)

keys = torch.rand(K, B * H * H, device="cuda", generator=g)
sort = timed({"gdl_sort_desc_f32": lambda: ops.sort_desc_f32(keys),
              "torch.sort": lambda: torch.sort(keys, dim=1, descending=True, stable=True)}, args.rounds, args.inner)
nbytes = keys.numel() * 20 * 4
for name, ts in sort.items():
    med = ts[len(ts) // 2]
    print(f"sort [{K}, {B * H * H}] {name:18s}: median {med:10.1f} us (min {ts[0]:.1f}, max {ts[-1]:.1f})"
          + (f"  {nbytes / med * 1e-3:7.1f} GB/s of {nbytes / 1e6:.0f} MB over 4 passes" if name.startswith("gdl") else ""))
