#!/usr/bin/env python
"""GPU micro-benchmark of UperNet's scale_modules stage (fpn1..fpn4 at the head of the decoder) at [B,36,36,768], bf16, HIP
events after warm-up: forward and forward + backward of the stage, and the achieved bytes/s (algorithmic traffic) of the new
elementwise kernels (BatchNorm -> GELU apply / backward sums / backward dx on the [B,72,72,384] map, 2x2 max-pool forward /
backward on [B,36,36,768]) next to the project's own bn_apply / bn_bwd_reduce / bn_bwd_dx on the same map in the same process.

    python tools/bench_scale_modules.py [B ...]      (default: 4 32)
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "geo-deep-learning_amd"))
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402
from geo_deep_learning.models.decoders.upernet import UperNetDecoder  # noqa: E402

bf = torch.bfloat16


def timeit(fn, rounds=7, inner=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    ts.sort()
    return ts[len(ts) // 2] * 1e3          # median, microseconds


def main():
    torch.manual_seed(0)
    dec = UperNetDecoder([768] * 4, align_corners=False, scale_modules=True).cuda().train()
    for B in [int(a) for a in sys.argv[1:]] or [4, 32]:
        xs = [torch.randn(B, 36, 36, 768, device="cuda").to(bf).requires_grad_() for _ in range(4)]
        outs = dec.scale_inputs_nhwc(xs)
        gs = [torch.randn_like(o) for o in outs]

        def fwd():
            with torch.no_grad():
                dec.scale_inputs_nhwc(xs)

        def fwd_bwd():
            for x in xs:
                x.grad = None
            dec.zero_grad(set_to_none=True)
            torch.autograd.backward(dec.scale_inputs_nhwc(xs), gs)
        print(f"B={B}: scale_modules stage forward {timeit(fwd):9.1f} us   forward+backward {timeit(fwd_bwd):9.1f} us")
        x = torch.randn(B, 72, 72, 384, device="cuda").to(bf)
        dy = torch.randn_like(x)
        c = x.shape[-1]
        g, b = torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda")
        mean, var = ops.bn_stats(x)
        out = torch.empty_like(x)
        sg, sb = ops.bn_gelu_bwd_reduce(x, dy, mean, var, g, b, 1e-5)
        p = x.numel() // c
        nb = x.numel() * 2
        rows = [
            ("bn_apply (ReLU, yardstick)", 2 * nb, lambda: ops.bn_apply(x, mean, var, g, b, 1e-5, True, out=out)),
            ("bn_gelu_apply", 2 * nb, lambda: ops.bn_gelu_apply(x, mean, var, g, b, 1e-5, out=out)),
            ("bn_bwd_reduce (ReLU, yardstick)", 2 * nb, lambda: ops.bn_bwd_reduce(x, dy, mean, var, g, b, 1e-5, True)),
            ("bn_gelu_bwd_reduce", 2 * nb, lambda: ops.bn_gelu_bwd_reduce(x, dy, mean, var, g, b, 1e-5)),
            ("bn_bwd_dx (ReLU, yardstick)", 3 * nb, lambda: ops.bn_bwd_dx(x, dy, mean, var, g, b, 1e-5, True, sg, sb, p, out=out)),
            ("bn_gelu_bwd_dx", 3 * nb, lambda: ops.bn_gelu_bwd_dx(x, dy, mean, var, g, b, 1e-5, sg, sb, p, out=out)),
        ]
        xm = torch.randn(B, 36, 36, 768, device="cuda").to(bf)
        ym = ops.maxpool2x2s2(xm)
        dm = torch.randn_like(ym)
        mb = xm.numel() * 2
        rows += [("maxpool2x2s2 fwd", mb + mb // 4, lambda: ops.maxpool2x2s2(xm)),
                 ("maxpool2x2s2 bwd", 2 * mb + mb // 4, lambda: ops.maxpool2x2s2_bwd(xm, dm))]
        for name, nbytes, fn in rows:
            us = timeit(fn)
            print(f"    {name:34s} {us:8.1f} us  {nbytes / us / 1e6:6.2f} TB/s  ({nbytes / 1e6:.1f} MB)")


if __name__ == "__main__":
    main()
