#!/usr/bin/env python
"""The probability tail of the exported inference model (tools/script_model.py) on one head map [B, 128, 128, K] -> 512^2 (the
main head of a DOFA model at 512^2 tiles), batch 64 by default.  us per call from HIP events around ``--inner`` calls, the variants
alternating round by round in one process:
  (a) upsample_probs                 -- gdl_upsample_probs, four pixels per thread (16-byte stores along Wo),
  (b) upsample_probs, 1 px / thread  -- the same entry point writing to a 4-byte-offset output: its one-pixel kernel,
  (c) upsample_logits + class_probs  -- what the wrapper ran before: the resized logits written, read, and the probabilities written.
(a) and (b) are checked against (c) before anything is timed.  Bytes: (a) / (b) write B*K*H*W*4 once; (c) moves three times that."""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "geo-deep-learning_amd"))
from gdlhip import _lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--classes", default="2,8")
ap.add_argument("--low", type=int, default=128)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--inner", type=int, default=20)
args = ap.parse_args()

B, h, H = args.batch, args.low, args.size
print(f"tools/bench_inference_tail.py --batch {B} --classes {args.classes} --low {h} --size {H} --rounds {args.rounds} --inner {args.inner}   "
      f"({torch.cuda.get_device_name(0)}, torch {torch.__version__})")
g = torch.Generator(device="cuda").manual_seed(0)
lib = _lib.load()


def timed(variants, rounds, inner):
    for fn in variants.values():      # warm-up: every variant
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


for K in (int(k) for k in args.classes.split(",")):
    low = torch.randn(B, h, h, K, device="cuda", generator=g) * 4
    n = B * K * H * H
    buf = torch.empty(n + 4, device="cuda")          # (b): an output one float past a 16-byte boundary

    def one_pixel():
        _lib.check(lib.gdl_upsample_probs(low.data_ptr(), B, h, h, K, buf[1:].data_ptr(), H, H, ops._stream()), "gdl_upsample_probs")
        return buf[1:n + 1].view(B, K, H, H)

    want = ops.class_probs(ops.upsample_logits(low, (H, H)))
    for name, got in (("(a)", ops.upsample_probs(low, (H, H))), ("(b)", one_pixel())):
        d = (got - want).abs().max().item()
        assert d <= 2.5e-7, (name, K, d)              # the same expressions; contraction may differ by an ulp of a probability
    variants = {"(a) upsample_probs": lambda: ops.upsample_probs(low, (H, H)), "(b) upsample_probs, 1 px / thread": one_pixel,
                "(c) upsample_logits + class_probs": lambda: ops.class_probs(ops.upsample_logits(low, (H, H)))}
    times = timed(variants, args.rounds, args.inner)
    ref = times["(c) upsample_logits + class_probs"][args.rounds // 2]
    print(f"K = {K}: [{B}, {h}, {h}, {K}] -> [{B}, {K}, {H}, {H}] f32 ({n * 4 / 2**20:.0f} MiB of probabilities); us per call, {args.rounds} rounds of {args.inner}")
    for name, ts in times.items():
        med = ts[len(ts) // 2]
        gbs = n * 4 * (3 if name.startswith("(c)") else 1) / (med * 1e-6) / 1e9
        print(f"  {name:36s} median {med:8.1f}  min {ts[0]:8.1f}  max {ts[-1]:8.1f}   ({med / ref:5.3f} x (c))   {gbs:7.0f} GB/s of tensor traffic")
print("the one-pass results agree with upsample_logits + class_probs to 2.5e-7")
