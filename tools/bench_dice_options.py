#!/usr/bin/env python
"""The Dice loss tail of one DOFA-base training step from the heads' low-resolution maps (both heads: 144^2 and 18^2 -> 512^2,
batch 64, 5 classes; forward + backward per head), us per step, for
  default        -- the plain entry points (gdl_dice_loss_lowres_fwd / _bwd),
  ignore unused  -- the option entry points with ignore_index=255 and a target without 255 (the cost of the `valid` test alone),
  ignore 20%     -- the same with a fifth of the pixels set to 255.
``--ab-lib PATH`` times the plain entry points of a second build of the library (for instance the parent commit's) in the same
process, alternating with this build's round by round, and compares loss, sums and gradients of the two bit for bit."""
import argparse
import ctypes as C
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "geo-deep-learning_amd"))
from gdlhip import _lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ab-lib", default=None)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--inner", type=int, default=20)
args = ap.parse_args()

B, K, H = args.batch, 5, 512
HEADS = (144, 18)
g = torch.Generator(device="cuda").manual_seed(0)
lows = [torch.randn(B, h, h, K, device="cuda", generator=g) * 2 for h in HEADS]
tgt = torch.randint(0, K, (B, H, H), device="cuda", generator=g)
tgt_ign = tgt.clone()
tgt_ign[torch.rand(B, H, H, device="cuda", generator=g) < 0.2] = 255
up = torch.tensor(0.4, device="cuda")
p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731


def bind(path):
    lib = C.CDLL(str(path))
    for name in ("gdl_dice_loss_lowres_workspace", "gdl_dice_loss_lowres_fwd", "gdl_dice_loss_lowres_bwd_workspace", "gdl_dice_loss_lowres_bwd"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def plain_tail(lib):
    """One step's loss tail through the plain entry points of ``lib``: [(loss, sums, dlow) per head]."""
    out, stream = [], C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for low, h in zip(lows, HEADS):
        sums, loss, dlow = torch.empty(3 * K, device="cuda"), torch.empty((), device="cuda"), torch.empty_like(low)
        n = lib.gdl_dice_loss_lowres_workspace(B, K, H, H)
        ws = torch.empty(n // 4, device="cuda")
        assert lib.gdl_dice_loss_lowres_fwd(p(low), p(tgt), B, K, h, h, H, H, 1e-7, p(sums), p(loss), p(ws), n, stream) == 0
        n = lib.gdl_dice_loss_lowres_bwd_workspace(B, K, h, h, H, H)
        ws2 = torch.empty(max(n // 4, 1), device="cuda")
        assert lib.gdl_dice_loss_lowres_bwd(p(low), p(tgt), B, K, h, h, H, H, 1e-7, p(sums), p(up), 1.0, p(dlow), p(ws2), n, stream) == 0
        out.append((loss, sums, dlow))
    return out


def option_tail(target, options):
    out = []
    for low in lows:
        loss, sums = ops.dice_loss_lowres_fwd(low, target, (H, H), options=options)
        out.append((loss, sums, ops.dice_loss_lowres_bwd(low, target, (H, H), sums, up, options=options)))
    return out


this = bind(_lib.LIB_PATH)
variants = {"default": lambda: plain_tail(this)}
if args.ab_lib:
    other = bind(args.ab_lib)
    variants["default, --ab-lib"] = lambda: plain_tail(other)
opt = ops.DiceOptions(ignore_index=255)
variants["ignore_index=255, unused"] = lambda: option_tail(tgt, opt)
variants["ignore_index=255, 20% ignored"] = lambda: option_tail(tgt_ign, opt)

for fn in variants.values():      # warm-up: every shape, every variant
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in variants}
for _ in range(args.rounds):      # the variants alternate round by round
    for name, fn in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) / args.inner * 1e3)
print(f"Dice loss tail from low-resolution logits, both heads ({HEADS[0]}^2 and {HEADS[1]}^2 -> {H}^2), batch {B}, K = {K}; "
      f"us per step, {args.rounds} rounds of {args.inner} steps")
base = sorted(times["default"])[args.rounds // 2]
for name, ts in times.items():
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    print(f"  {name:32s} median {med:8.1f}  min {ts[0]:8.1f}  max {ts[-1]:8.1f}   ({med / base:5.3f} x default)")
same = all(torch.equal(a, b) for x, y in zip(plain_tail(this), option_tail(tgt, opt)) for a, b in zip(x, y))
print(f"option entry points with an unused ignore_index == plain entry points, bit for bit: {same}")
if args.ab_lib:
    same_ab = all(torch.equal(a, b) for x, y in zip(plain_tail(this), plain_tail(other)) for a, b in zip(x, y))
    print(f"plain entry points == --ab-lib's, bit for bit (loss, sums, d low; both heads): {same_ab}")
    assert same_ab
assert same
