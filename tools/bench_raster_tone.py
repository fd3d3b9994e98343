#!/usr/bin/env python
"""Raster radiometry (include/gdlhip_raster_tone.h): ``ops.raster_hist`` and ``ops.raster_stretch`` at a scene-sized shape.

The source is a ``--bands``-band uint16 raster of ``--side`` x ``--side`` pixels (3 x 8192^2 by default: 403 MB) in two fillings:
uniform random 11-bit values, and one constant value (every lane of a wave adds to one LDS counter: the worst case of the
histogram).  The histogram's yardstick is ``ops.raster_stats`` on the same raster, which reads the same bytes once; the
stretch's is the bytes it moves (2 B in and 1 B out per sample) against a device-to-device copy of as many bytes timed in the same
process.  The quantiles (one small launch per band) are timed too.  ms per call from HIP events around ``--inner`` calls, the
best of ``--rounds`` rounds, after a warm-up call.  One JSON line per measurement."""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "geo-deep-learning_amd"))
from gdlhip import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=8192)
ap.add_argument("--bands", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--inner", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_raster_tone needs a GPU"
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
    print(json.dumps({"what": what, "ms": round(ms, 3), "GB": round(nbytes / 1e9, 3), "GB/s": round(nbytes / ms / 1e6, 1), **more}), flush=True)


side, bands = args.side, args.bands
g = torch.Generator(device=dev).manual_seed(5)
fillings = {"random 11-bit": torch.randint(0, 2048, (bands, side, side), device=dev, dtype=torch.int16, generator=g).view(torch.uint16),
            "constant": torch.full((bands, side, side), 1000, device=dev, dtype=torch.int16).view(torch.uint16)}
src_bytes = bands * side * side * 2
for name, raster in fillings.items():
    stats_ms = timed(lambda: ops.raster_stats(raster, None, ops.RasterStats()))
    report(f"raster_stats uint16, {name}", stats_ms, src_bytes)
    hist = ops.raster_hist(raster)
    acc = torch.zeros_like(hist.acc)
    keep = ops.RasterHist(raster.dtype, bands, hist.bins)
    keep.acc = acc      # one accumulator for every call: the time is the kernel's, not an allocation's
    ms = timed(lambda: ops.raster_hist(raster, None, keep))
    report(f"raster_hist uint16, {name}", ms, src_bytes, of_stats=round(ms / stats_ms, 2), bins_hit=int((hist.counts[0] != 0).sum()))
    report(f"quantiles (2 per band), {name}", timed(lambda: hist.percentile_bounds(2.0, 98.0)), hist.acc.numel() * 8)
    bounds = hist.percentile_bounds(2.0, 98.0)
    moved = bands * side * side * 3
    ms = timed(lambda: ops.raster_stretch(raster, bounds, (1, 255)))
    cms = copy_ms(moved)
    report(f"raster_stretch uint16 -> uint8, {name}", ms, moved, copy_ms=round(cms, 3), copy_GBps=round(moved / cms / 1e6, 1),
           of_copy=round(cms / ms, 3))
