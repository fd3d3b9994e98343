#!/usr/bin/env python
"""Whole-scene inference (tools/scene_inference.py, include/gdlhip_scene.h, include/gdlhip_scene_tta.h,
include/gdlhip_scene_nodata.h, include/gdlhip_scene_sieve.h, include/gdlhip_scene_rings.h), six measurements in one process.

1. The tail of one batch of 64 tiles of 512^2 at stride 256 (an 8 x 8 grid over a 2304^2 uint8 scene), K = 5, the model excluded:
   its head map [64, 128, 128, 5] is drawn once.  ms per batch from HIP events around ``--inner`` repetitions, the variants
   alternating round by round:
     (a) fused, low-resolution  -- scene_cut, scene_blend_lowres, scene_finish (what SceneInference runs),
     (b) fused, full-resolution -- scene_cut, upsample_probs, scene_blend, scene_finish (its route for a model without head maps),
     (c) composed               -- what the code allowed before: a host loop of 64 slice copies, normalize_range, upsample_probs,
                                   a torch multiply by the window, 64 indexed adds into the canvas, a divide and an argmax.
   Every variant zeroes its canvas first; (a) and (b) are compared with (c) before anything is timed.
1b. The same tail with test-time augmentation: one batch of 64 (tile, transform) pairs, for three sets of codes -- "flips"
   (16 tiles x codes 0..3), "transposing" (16 tiles x codes 4..7) and "d4" (8 tiles x all eight) -- the model excluded as above
   (its head map of the transformed tiles is drawn once):
     (a) fused, low-resolution  -- scene_cut_d4, scene_blend_lowres_d4, scene_finish (what SceneInference(tta=...) runs),
     (b) fused, full-resolution -- scene_cut_d4, upsample_probs, scene_blend_d4, scene_finish,
     (c) composed               -- from the pieces without a transform: scene_cut, one torch flip / transpose copy per code into
                                   the model's batch, upsample_probs, one torch inverse permutation copy per code, scene_blend,
                                   scene_finish.
   (b) must equal (c) to the bit and (a) agree with it before anything is timed.
2. SceneInference on a synthetic 4096^2 scene (15 x 15 = 225 tiles) with the DOFA-base model in bf16, as tiles per second of the
   whole call, next to ScriptModel's tiles per second on the same tiles (batches of host-sliced tiles, probabilities written).
3. The same scene and model with a nodata border: the samples outside a centred square are 0 in every band, the border taking
   ``--nodata-share`` of the pixels.  Seconds per scene of ``SceneInference.predict`` without ``nodata=`` (every tile is fed) and
   with ``nodata=0`` (scene_valid, scene_tile_valid, the tiles without data dropped, scene_cut_valid, scene_finish_valid), the two
   alternating, with the tiles kept of the total; the masks are compared on the valid pixels first.
4. ``ops.scene_sieve`` alone on a label mask of the scene's size (``--scene``, 4096 where that is 0): K classes in blocks of 64^2
   with 2 % of the pixels redrawn at random, sieved at ``--sieve`` pixels, connectivity 4 and 8.  ms per call from HIP events, the
   bytes its kernels move per pixel (from the shapes) as GB/s and as a share of the HBM rate, and beside it the seconds
   ``scipy.ndimage.label`` needs on the host for the labelling alone of the same mask (where scipy is there).
5. ``ops.scene_rings`` on a ``--rings`` x ``--rings`` mask, for two inputs: site percolation at the threshold (p = 0.5927) sieved at
   ``--sieve`` pixels (64 where that is 0), and a constant mask.  The counts E (boundary sides), R (rings) and V (vertices), ms of
   the whole call on the host clock (it holds two device-to-host copies and the allocations), and ms of each stage from HIP
   events around its entry point alone: gdl_scene_components, gdl_scene_rings_count, _trace and _write."""
import argparse
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "geo-deep-learning_amd"))
from gdlhip import ops  # noqa: E402
from gdlhip import scene as gscene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--classes", type=int, default=5)
ap.add_argument("--tile", type=int, default=512)
ap.add_argument("--stride", type=int, default=256)
ap.add_argument("--grid", type=int, default=8, help="tiles per side of the batch (8 x 8 = 64)")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--scene", type=int, default=4096, help="side of the whole scene of part 2 (0 = skip part 2)")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--scene-repeats", type=int, default=3)
ap.add_argument("--no-tta", action="store_true", help="skip part 1b")
ap.add_argument("--nodata-share", type=float, default=0.4, help="share of the scene of part 3 that is a nodata border (0 = skip part 3)")
ap.add_argument("--sieve", type=int, default=64, help="minimum mapping unit of part 4 in pixels (0 = skip part 4)")
ap.add_argument("--rings", type=int, default=8192, help="side of the mask of part 5 (0 = skip part 5)")
ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate part 4 compares with, GB/s")
args = ap.parse_args()

K, T, S = args.classes, args.tile, args.stride
side = T + S * (args.grid - 1)
print(f"tools/bench_scene.py --classes {K} --tile {T} --stride {S} --grid {args.grid} --rounds {args.rounds} --inner {args.inner} "
      f"--scene {args.scene} --batch {args.batch}   ({torch.cuda.get_device_name(0)}, torch {torch.__version__})")
g = torch.Generator(device="cuda").manual_seed(0)
mean, std = torch.tensor([0.485, 0.456, 0.406], device="cuda"), torch.tensor([0.229, 0.224, 0.225], device="cuda")
RANGE = (0, 255, 0.0, 1.0)

# ------------------------------------------------------------------ 1. the tail of one batch
raster = torch.randint(0, 256, (3, side, side), device="cuda", dtype=torch.uint8, generator=g)
plan = gscene.plan_tiles(side, side, (T, T), (S, S))
B = plan.shape[0]
assert B == args.grid ** 2
origins, box, where = plan.cuda(), gscene.bounding_box(plan, (T, T)), plan.tolist()
low = torch.randn(B, T // 4, T // 4, K, device="cuda", generator=g) * 4
wy = wx = gscene.window(T, "hann").cuda()
w2 = wy[:, None] * wx[None, :]
canvas = torch.zeros(K + 1, side, side, device="cuda")


def fused_lowres():
    canvas.zero_()
    ops.scene_cut(raster, origins, (T, T), mean, std, *RANGE)
    ops.scene_blend_lowres(low, (T, T), origins, wy, wx, canvas, box)
    return ops.scene_finish(canvas)[0]


def fused_full():
    canvas.zero_()
    ops.scene_cut(raster, origins, (T, T), mean, std, *RANGE)
    ops.scene_blend(ops.upsample_probs(low, (T, T)), origins, wy, wx, canvas, box)
    return ops.scene_finish(canvas)[0]


def composed():
    canvas.zero_()
    ops.normalize_range(torch.stack([raster[:, y:y + T, x:x + T] for y, x in where]), mean, std, *RANGE)
    weighted = ops.upsample_probs(low, (T, T)) * w2
    for t, (y, x) in enumerate(where):
        canvas[:K, y:y + T, x:x + T] += weighted[t]
        canvas[K, y:y + T, x:x + T] += w2
    return (canvas[:K] / canvas[K]).argmax(0)


def timed(variants, rounds, inner):
    for fn in variants.values():      # warm-up: every variant
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
            times[name].append(e0.elapsed_time(e1) / inner)
    return {k: sorted(v) for k, v in times.items()}


want_mask = composed()
want_canvas = canvas.clone()
for name, fn in (("(a)", fused_lowres), ("(b)", fused_full)):
    mask = fn()
    d = (canvas - want_canvas).abs().max().item()
    differ = (mask.long() != want_mask).float().mean().item()
    print(f"{name} vs (c): canvas max |diff| {d:.3e} (sums of up to four weighted probabilities), labels that differ {differ:.2e} of the pixels")
    assert d <= 1e-5 and differ <= 1e-4, (name, d, differ)

MIB = 2 ** 20
px, tile_px = side * side, B * T * T
# bytes each route moves through HBM-visible tensors, from the shapes (the maps and windows, a few MiB, left out)
cut = tile_px * 3 * (1 + 4)      # one raw byte read and one f32 written per tile value
bytes_fused = cut + 2 * (K + 1) * px * 4 + (K + 1) * px * 4 + px + (K + 1) * px * 4      # cut, blend read + write, finish read + mask, zero fill
bytes_full = bytes_fused + 2 * tile_px * K * 4      # + the probabilities written and read
bytes_composed = (2 * tile_px * 3 + tile_px * 3 + tile_px * 3 * 4 + 3 * tile_px * K * 4      # slices, normalise, probabilities, x window
                  + 3 * tile_px * (K + 1) * 4 + 3 * K * px * 4 + K * px * 4 + 8 * px + (K + 1) * px * 4)      # adds, divide, argmax, zero fill
times = timed({"(a) fused, low-resolution": fused_lowres, "(b) fused, full-resolution": fused_full, "(c) composed": composed}, args.rounds, args.inner)
ref = times["(c) composed"][args.rounds // 2]
print(f"tail of one batch: {B} tiles of {T}^2 at stride {S} over {side}^2, K = {K}; ms per batch, {args.rounds} rounds of {args.inner}")
for (name, ts), nbytes in zip(times.items(), (bytes_fused, bytes_full, bytes_composed)):
    med = ts[len(ts) // 2]
    print(f"  {name:28s} median {med:8.3f}  min {ts[0]:8.3f}  max {ts[-1]:8.3f}   ({med / ref:5.3f} x (c))   {nbytes / MIB:7.0f} MiB of tensor traffic, "
          f"{nbytes / (med * 1e-3) / 1e9:6.0f} GB/s")
del raster, low, canvas, want_canvas, want_mask

# ------------------------------------------------------------------ 1b. the tail of one batch of (tile, transform) pairs
def tta_tail(label, grid, codes):
    """Times the three variants for ``grid`` = (rows, columns) of tiles, each with the transforms ``codes``."""
    G = len(codes)
    h, w = T + S * (grid[0] - 1), T + S * (grid[1] - 1)
    raster = torch.randint(0, 256, (3, h, w), device="cuda", dtype=torch.uint8, generator=g)
    tiles_plan = gscene.plan_tiles(h, w, (T, T), (S, S))
    plan, xf = gscene.plan_tta(tiles_plan, codes)
    B = plan.shape[0]
    assert B == grid[0] * grid[1] * G
    origins, xforms, box = plan.cuda(), xf.cuda(), gscene.bounding_box(plan, (T, T))
    low = torch.randn(B, T // 4, T // 4, K, device="cuda", generator=g) * 4      # the head's maps of the transformed tiles
    canvas = torch.zeros(K + 1, h, w, device="cuda")

    def fused_lowres():
        canvas.zero_()
        ops.scene_cut_d4(raster, origins, xforms, (T, T), mean, std, *RANGE, check_codes=False)
        ops.scene_blend_lowres_d4(low, (T, T), origins, xforms, wy, wx, canvas, box, check_codes=False)
        return ops.scene_finish(canvas)[0]

    def fused_full():
        canvas.zero_()
        ops.scene_cut_d4(raster, origins, xforms, (T, T), mean, std, *RANGE, check_codes=False)
        ops.scene_blend_d4(ops.upsample_probs(low, (T, T)), origins, xforms, wy, wx, canvas, box, check_codes=False)
        return ops.scene_finish(canvas)[0]

    def composed():
        canvas.zero_()
        cut = ops.scene_cut(raster, origins, (T, T), mean, std, *RANGE)
        fed = torch.empty_like(cut)                      # the model's batch: pair j of every tile is its j-th transform
        for j, code in enumerate(codes):
            fed[j::G] = gscene.d4_apply(cut[j::G], code)
        probs = ops.upsample_probs(low, (T, T))
        back = torch.empty_like(probs)
        for j, code in enumerate(codes):
            back[j::G] = gscene.d4_apply(probs[j::G], gscene.d4_inverse(code))
        ops.scene_blend(back, origins, wy, wx, canvas, box)
        return ops.scene_finish(canvas)[0]

    want_mask = composed()
    want_canvas = canvas.clone()
    cut_want = torch.empty(B, 3, T, T, device="cuda")
    plain = ops.scene_cut(raster, origins, (T, T), mean, std, *RANGE)
    for j, code in enumerate(codes):
        cut_want[j::G] = gscene.d4_apply(plain[j::G], code)
    assert torch.equal(ops.scene_cut_d4(raster, origins, xforms, (T, T), mean, std, *RANGE), cut_want), label
    del cut_want, plain
    mask = fused_full()
    assert torch.equal(canvas, want_canvas) and torch.equal(mask, want_mask), f"{label}: (b) differs from (c)"
    mask = fused_lowres()
    d = (canvas - want_canvas).abs().max().item()
    differ = (mask != want_mask).float().mean().item()
    print(f"TTA {label}: (b) equals (c) to the bit; (a) vs (c): canvas max |diff| {d:.3e} (sums of up to {4 * G} weighted probabilities), "
          f"labels that differ {differ:.2e} of the pixels")
    assert d <= 1e-5 * G and differ <= 1e-4, (label, d, differ)

    px, tile_px = h * w, B * T * T
    cut_b = tile_px * 3 * (1 + 4)
    b_fused = cut_b + 2 * (K + 1) * px * 4 + (K + 1) * px * 4 + px + (K + 1) * px * 4      # as in part 1: nothing is added by the transform
    b_full = b_fused + 2 * tile_px * K * 4
    b_composed = b_full + 2 * tile_px * 3 * 4 + 2 * tile_px * K * 4      # + the tiles and the probabilities read and written once more
    times = timed({"(a) fused, low-resolution": fused_lowres, "(b) fused, full-resolution": fused_full, "(c) composed": composed},
                  args.rounds, args.inner)
    ref = times["(c) composed"][args.rounds // 2]
    print(f"TTA tail of one batch, {label}: {B} pairs = {B // G} tiles of {T}^2 at stride {S} over {h} x {w}, codes {tuple(codes)}, K = {K}; "
          f"ms per batch, {args.rounds} rounds of {args.inner}")
    for (name, ts), nbytes in zip(times.items(), (b_fused, b_full, b_composed)):
        med = ts[len(ts) // 2]
        print(f"  {name:28s} median {med:8.3f}  min {ts[0]:8.3f}  max {ts[-1]:8.3f}   ({med / ref:5.3f} x (c))   {nbytes / MIB:7.0f} MiB of tensor traffic, "
              f"{nbytes / (med * 1e-3) / 1e9:6.0f} GB/s")


if not args.no_tta:
    tta_tail("flips", (4, 4), gscene.FLIPS)
    tta_tail("transposing", (4, 4), (4, 5, 6, 7))
    tta_tail("d4", (2, 4), gscene.D4)

# ------------------------------------------------------------------ 2. a whole scene through the model
if args.scene:
    from geo_deep_learning.models.segmentation.dofa import DOFASegmentationModel
    from geo_deep_learning.tools.scene_inference import SceneInference
    from geo_deep_learning.tools.script_model import SegmentationScriptModel

    torch.manual_seed(0)
    model = DOFASegmentationModel(encoder="dofa_base", image_size=(T, T), freeze_layers=["encoder"], num_classes=K, pretrained=False)
    sm = SegmentationScriptModel(model, wavelengths=torch.tensor([0.665, 0.560, 0.490]), device=torch.device("cuda"), num_classes=K,
                                 input_shape=(1, 3, T, T), mean=mean.tolist(), std=std.tolist(), bf16=True)
    scene = torch.randint(0, 256, (3, args.scene, args.scene), dtype=torch.uint8)
    si = SceneInference(sm, tile=(T, T), stride=(S, S), batch_size=args.batch)
    tiles = gscene.plan_tiles(args.scene, args.scene, (T, T), (S, S)).tolist()

    def whole_scene():
        return si.predict(scene).mask

    def tile_by_tile():
        dev = scene.cuda()
        for i in range(0, len(tiles), args.batch):
            sm(torch.stack([dev[:, y:y + T, x:x + T] for y, x in tiles[i:i + args.batch]]))

    for name, fn in (("SceneInference.predict (upload, cut, model, blend, finish)", whole_scene),
                     ("ScriptModel on the same tiles (upload, slices, model, probabilities)", tile_by_tile)):
        fn()      # warm-up: every shape of the timed call, the short last batch included
        torch.cuda.synchronize()
        rates = []
        for _ in range(args.scene_repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rates.append(len(tiles) / (time.perf_counter() - t0))
        rates.sort()
        print(f"scene {args.scene}^2, {len(tiles)} tiles, batch {args.batch}, bf16 DOFA-base: {name}: median {rates[len(rates) // 2]:7.1f} tiles/s  "
              f"(min {rates[0]:7.1f}, max {rates[-1]:7.1f}; {args.scene_repeats} runs)")

    # -------------------------------------------------------------- 3. the same scene inside a nodata border
    if args.nodata_share > 0:
        n = args.scene
        inner = round(n * (1.0 - args.nodata_share) ** 0.5)      # the side of the centred square that holds data
        lo = (n - inner) // 2
        bordered = torch.zeros_like(scene)
        bordered[:, lo:lo + inner, lo:lo + inner] = scene[:, lo:lo + inner, lo:lo + inner].clamp(min=1)
        share = 1.0 - inner * inner / (n * n)
        si_nd = SceneInference(sm, tile=(T, T), stride=(S, S), batch_size=args.batch, nodata=0)
        kept, counts = si_nd.tile_plan(bordered)
        data = (bordered != 0).any(0).cuda()
        every, skipping = si.predict(bordered).mask, si_nd.predict(bordered).mask
        assert torch.equal(every[data], skipping[data]) and (skipping[~data] == 255).all(), "nodata= changes a valid pixel"
        variants = {"without nodata= (every tile fed)": lambda: si.predict(bordered).mask, "with nodata=0 (empty tiles dropped)": lambda: si_nd.predict(bordered).mask}
        secs = {k: [] for k in variants}
        for _ in range(args.scene_repeats):      # both are warm: the comparison above ran them
            for name, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                secs[name].append(time.perf_counter() - t0)
        print(f"scene {n}^2 with a nodata border of {share:.1%} of the pixels (data in the centred {inner}^2), batch {args.batch}, bf16 DOFA-base: "
              f"{kept.shape[0]} of {counts.shape[0]} tiles hold data")
        base = sorted(secs["without nodata= (every tile fed)"])[args.scene_repeats // 2]
        for name, ts in secs.items():
            ts.sort()
            print(f"  SceneInference.predict {name:36s} median {ts[len(ts) // 2]:7.3f} s  (min {ts[0]:7.3f}, max {ts[-1]:7.3f}; {args.scene_repeats} runs)   "
                  f"{ts[len(ts) // 2] / base:5.3f} x")

# ------------------------------------------------------------------ 4. the sieve alone
if args.sieve > 0:
    n = args.scene or 4096
    gs = torch.Generator().manual_seed(4)
    blocks = torch.randint(0, K, ((n + 63) // 64, (n + 63) // 64), generator=gs, dtype=torch.uint8)
    label_mask = blocks.repeat_interleave(64, 0).repeat_interleave(64, 1)[:n, :n].contiguous()
    noise = torch.rand((n, n), generator=gs) < 0.02
    label_mask[noise] = torch.randint(0, K, (int(noise.sum()),), generator=gs, dtype=torch.uint8)
    dev_mask = label_mask.cuda()
    # per pixel: the tile kernel reads the mask and writes parents and zeroed sizes (1 + 4 + 4), the flattening reads and writes the
    # labels (4 + 4), the clearing reads the sizes (4), the vote reads mask, labels and sizes (1 + 4 + 4) and the rewrite the same
    # and writes the mask (1 + 4 + 4 + 1); the unions across tile edges and the atomics touch a few per cent of that
    sieve_bytes = 9 + 8 + 4 + 9 + 10
    for connectivity in (4, 8):
        variants = {f"scene_sieve, connectivity {connectivity}": lambda c=connectivity: ops.scene_sieve(dev_mask, args.sieve, c),
                    f"scene_components alone, connectivity {connectivity}": lambda c=connectivity: ops.scene_components(dev_mask, c)}
        out = ops.scene_sieve(dev_mask, args.sieve, connectivity)
        changed = int((out != dev_mask).sum())
        times = timed(variants, args.rounds, args.inner)
        print(f"sieve of a {n}^2 mask, K = {K}, min_size {args.sieve}, connectivity {connectivity}: {changed} pixels changed; ms per call, "
              f"{args.rounds} rounds of {args.inner}")
        for (name, ts), nbytes in zip(times.items(), (sieve_bytes, 17)):
            med = ts[len(ts) // 2]
            rate = nbytes * n * n / (med * 1e-3) / 1e9
            print(f"  {name:40s} median {med:8.3f}  min {ts[0]:8.3f}  max {ts[-1]:8.3f}   {nbytes} B per pixel, {rate:6.0f} GB/s, "
                  f"{rate / args.hbm_gbs:6.1%} of {args.hbm_gbs:.0f} GB/s")
    try:
        from scipy import ndimage
    except ImportError:
        print("  scipy is not installed: no host time beside it")
    else:
        host = label_mask.numpy()
        t0 = time.perf_counter()
        for value in range(K):
            ndimage.label(host == value)
        print(f"  scipy.ndimage.label on the host, the {K} classes one after the other (labelling alone, connectivity 4): "
              f"{time.perf_counter() - t0:.2f} s")

# ------------------------------------------------------------------ 5. the polygon rings
if args.rings > 0:
    from gdlhip import _lib
    n = args.rings
    lib, stream = _lib.checked(), torch.cuda.current_stream().cuda_stream
    percolation = (torch.rand((n, n), generator=torch.Generator().manual_seed(5)) < 0.5927).to(torch.uint8).cuda()
    inputs = {f"percolation (p = 0.5927) sieved at {args.sieve or 64} pixels": ops.scene_sieve(percolation, args.sieve or 64, 4),
              "constant": torch.full((n, n), 3, dtype=torch.uint8, device="cuda")}
    del percolation

    def i32(count):
        return torch.empty((count,), device="cuda", dtype=torch.int32)

    def blocks(count):
        return -(-count // _lib.SCENE_RINGS_SCAN_TILE)

    def stages(mask, connectivity):
        """ops.scene_rings call by call, every entry point between two HIP events of its own: ({stage: ms}, (E, R, V))."""
        ms, keep = {}, torch.ones(256, dtype=torch.uint8, device="cuda")

        def p(x):
            return x.data_ptr()

        def run(name, fn, *a):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn(*a, stream)
            end.record()
            end.synchronize()
            ms[name] = start.elapsed_time(end)

        labels, sizes, offsets, n_sides, counts = torch.empty((n, n), device="cuda", dtype=torch.int32), i32(n * n), i32(n * n), i32(1), i32(2)
        run("gdl_scene_components", lib.gdl_scene_components, p(mask), n, n, connectivity, -1, p(labels), p(sizes))
        del sizes
        run("gdl_scene_rings_count", lib.gdl_scene_rings_count, p(mask), n, n, -1, p(keep), p(offsets), p(i32(blocks(n * n))), p(n_sides))
        E = int(n_sides.item())
        side = [i32(E) for _ in range(4)]
        work = i32(3 * E + 2 * blocks(E) + _lib.SCENE_RINGS_FLAGS)
        run("gdl_scene_rings_trace", lib.gdl_scene_rings_trace, p(mask), n, n, connectivity, -1, p(keep), p(offsets), E, *map(p, side), p(work),
            p(counts))
        R, V = counts.tolist()
        out = (torch.empty((V, 2), device="cuda", dtype=torch.int32), i32(R + 1), torch.empty((R,), device="cuda", dtype=torch.uint8),
               i32(R), i32(R), torch.empty((R,), device="cuda", dtype=torch.int64))
        run("gdl_scene_rings_write", lib.gdl_scene_rings_write, p(mask), p(labels), n, E, R, V, *map(p, side), p(work), *map(p, out))
        return ms, (E, R, V)

    for name, mask in inputs.items():
        for connectivity in (4, 8):
            whole = ops.scene_rings(mask, connectivity)      # warm-up, and what the stages must add up to
            runs, clock = [], []
            for _ in range(args.rounds):
                runs.append(stages(mask, connectivity))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ops.scene_rings(mask, connectivity)
                torch.cuda.synchronize()
                clock.append((time.perf_counter() - t0) * 1e3)
            E, R, V = runs[0][1]
            assert (R, V) == (whole.value.numel(), whole.vertices.shape[0]) and all(r[1] == (E, R, V) for r in runs)
            clock.sort()
            print(f"rings of a {n}^2 mask, {name}, connectivity {connectivity}: E = {E} sides, R = {R} rings, V = {V} vertices, "
                  f"{max(E - 1, 0).bit_length()} doubling rounds at the most; ms, {args.rounds} runs")
            print(f"  {'ops.scene_rings, whole call (host clock)':44s} median {clock[len(clock) // 2]:9.3f}  min {clock[0]:9.3f}  max {clock[-1]:9.3f}")
            for stage in runs[0][0]:
                ts = sorted(r[0][stage] for r in runs)
                print(f"  {stage:44s} median {ts[len(ts) // 2]:9.3f}  min {ts[0]:9.3f}  max {ts[-1]:9.3f}")
            del whole
