#!/usr/bin/env python
"""Raster preparation (include/gdlhip_raster.h): achieved GB/s of ``ops.raster_warp`` and ``ops.raster_stats`` at a scene-sized
shape, next to a device-to-device copy timed in the same process.

The source is a ``--bands``-band uint16 raster of ``--side`` x ``--side`` pixels (4 x 10 000^2 by default: 800 MB) with a nodata
border.  Three geometries -- the same resolution shifted by half a pixel, the 2x upsample (scale 0.5) and 2.5x coarser (scale 2.5)
-- each with nearest, bilinear and cubic, uint16 out, validity planes not written; then the statistics pass over the same raster.
ms per call from HIP events around ``--inner`` calls, the best of ``--rounds`` rounds.  Bytes: what the call has to move once,
the source read plus the destination written (the statistics: the source read), from the shapes; GB/s = bytes / time.  The
yardstick is ``Tensor.copy_`` between two device buffers of half those bytes (it reads and writes as many bytes as the call moves),
timed the same way right after the call it is compared with.  One JSON line per measurement."""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "geo-deep-learning_amd"))
from gdlhip import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=10000)
ap.add_argument("--bands", type=int, default=4)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--inner", type=int, default=3)
ap.add_argument("--methods", default="nearest,bilinear,cubic")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_raster needs a GPU"
dev = "cuda"


def timed(fn) -> float:
    """ms per call: the best round of --rounds, each --inner calls between two events, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / args.inner)
    return best


def copy_ms(total_bytes: int) -> float:
    """A device-to-device copy that reads total_bytes / 2 and writes total_bytes / 2."""
    n = max(total_bytes // 2, 1)
    src, dst = torch.empty(n, device=dev, dtype=torch.uint8), torch.empty(n, device=dev, dtype=torch.uint8)
    src.zero_()
    ms = timed(lambda: dst.copy_(src))
    del src, dst
    return ms


def report(what: str, ms: float, nbytes: int, **more) -> None:
    cms = copy_ms(nbytes)
    print(json.dumps({"what": what, "ms": round(ms, 3), "GB": round(nbytes / 1e9, 3), "GB/s": round(nbytes / ms / 1e6, 1),
                      "copy_ms": round(cms, 3), "copy_GB/s": round(nbytes / cms / 1e6, 1), "of_copy": round(cms / ms, 3), **more}), flush=True)


side, bands = args.side, args.bands
g = torch.Generator(device=dev).manual_seed(5)
base = torch.randint(1, 4096, (bands, side, side), device=dev, dtype=torch.int16, generator=g)
border = max(side // 50, 1)
base[:, :border], base[:, -border:], base[:, :, :border], base[:, :, -border:] = 0, 0, 0, 0
raster = base.view(torch.uint16)      # values below 2^15: the same bits
src_bytes = raster.numel() * 2

geometries = {"shift": (1.0, 0.5, side), "up2": (0.5, 0.0, 2 * side), "coarser2.5": (2.5, 0.0, int(side / 2.5))}
for name, (s, o, n) in geometries.items():
    for method in args.methods.split(","):
        out = ops.raster_warp(raster, (n, n), s, o, s, o, method, nodata=0, dst_nodata=0)
        valid_share = float((out.view(torch.int16) != 0).float().mean())
        del out
        ms = timed(lambda: ops.raster_warp(raster, (n, n), s, o, s, o, method, nodata=0, dst_nodata=0))
        report(f"raster_warp {name} {method}", ms, src_bytes + bands * n * n * 2, dst=[bands, n, n], scale=s, valid_share=round(valid_share, 4))

stats = ops.raster_stats(raster, 0)
means, stds = stats.finish()
ms = timed(lambda: ops.raster_stats(raster, 0, ops.RasterStats()))
report("raster_stats uint16", ms, src_bytes, mean0=round(means[0], 3), std0=round(stds[0], 3))
as_float = base[:1].float()
ms = timed(lambda: ops.raster_stats(as_float, 0.0, ops.RasterStats()))
report("raster_stats float32 (one band)", ms, as_float.numel() * 4)
