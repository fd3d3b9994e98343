"""Worker of tests/test_hip_scale_modules.py (own process): `graph` -- decoder training step captured in a hipGraph against
eager steps; `sync` -- ConvTranspose -> SyncBatchNorm -> GELU at world size 2 on one GPU.  Prints one JSON line."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "geo-deep-learning_amd", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import torch  # noqa: E402
from torch import nn  # noqa: E402

from _scale_modules_recipe import load_golden, recipe_inputs  # noqa: E402
from gdlhip import nn as gnn  # noqa: E402
from geo_deep_learning.models.decoders.upernet import UperNetDecoder  # noqa: E402
from oracle import procedural_state_dict  # noqa: E402

DEV = "cuda"


def _decoder(meta):
    dec = UperNetDecoder([meta["embed"]] * 4, channels=meta["channels"], align_corners=False, scale_modules=True)
    dec.load_state_dict(procedural_state_dict(dec, meta["seed"]))
    return dec.to(DEV).train()


def graph_main():
    _, meta = load_golden()
    xs, g = recipe_inputs(meta)
    xs, g = [x.to(DEV) for x in xs], (g * 512).to(DEV).contiguous(memory_format=torch.channels_last)

    def step(dec, opt, zero=True):
        if zero:
            opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = dec(xs)
        (out.float() * g).sum().backward()
        opt.step()
        return out

    de, dg = _decoder(meta), _decoder(meta)
    oe = gnn.FusedAdam(list(de.parameters()), lr=1e-2, capturable=True)
    og = gnn.FusedAdam(list(dg.parameters()), lr=1e-2, capturable=True)
    warm = 2
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm):
            step(dg, og)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(warm):
        step(de, oe)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    og.zero_grad(set_to_none=True)          # gradients are (re)allocated from the graph's private pool
    with torch.cuda.graph(graph):
        static_out = step(dg, og, zero=False)
    keep = [entry[1] for entry in list(gnn._CACHE.values())]      # operands the captured kernels read through their address
    first = None
    equal = []
    for i in range(3):
        graph.replay()
        og.note_replay()
        want = step(de, oe).detach()
        torch.cuda.synchronize()
        equal.append(bool(torch.equal(static_out.detach(), want)))
        first = want.clone() if first is None else first
    params_equal = all(torch.equal(a, b) for a, b in zip(de.parameters(), dg.parameters()))
    bufs_equal = all(torch.equal(a, b) for a, b in zip(de.buffers(), dg.buffers()))
    print(json.dumps({"replays": 3, "outputs_equal": equal, "params_equal": params_equal and bufs_equal,
                      "moved": not torch.equal(first, want), "kept": len(keep)}))


def _sync_case():
    g = torch.Generator().manual_seed(77)
    x = torch.randn(4, 6, 5, 32, generator=g)
    gy = torch.randn(4, 12, 10, 16, generator=g)
    convt, bn = nn.ConvTranspose2d(32, 16, 2, 2), nn.BatchNorm2d(16)
    with torch.no_grad():
        convt.weight.copy_(torch.randn(32, 16, 2, 2, generator=g) * 0.25)
        convt.bias.copy_(torch.randn(16, generator=g) * 0.1)
        bn.weight.copy_(1 + 0.2 * torch.randn(16, generator=g))
        bn.bias.copy_(0.3 * torch.randn(16, generator=g))
    return x, gy, convt, bn


def _sync_worker(rank, world, port, ret):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x, gy, convt, bn = _sync_case()
        convt = convt.to(DEV).train()
        bn = nn.SyncBatchNorm.convert_sync_batchnorm(bn).to(DEV).train()
        lo, hi = 2 * rank, 2 * rank + 2
        xd = x[lo:hi].to(DEV).requires_grad_()
        out = gnn.conv_transpose2x2_bn_gelu(xd, convt, bn)
        out.backward(gy[lo:hi].to(DEV))
        torch.cuda.synchronize()
        ret[rank] = {"out": out.detach().cpu(), "dx": xd.grad.cpu(), "dw": convt.weight.grad.cpu(), "dgamma": bn.weight.grad.cpu(),
                     "dbeta": bn.bias.grad.cpu(), "rm": bn.running_mean.cpu(), "rv": bn.running_var.cpu(),
                     "nbt": int(bn.num_batches_tracked), "msgs": list(gnn.SYNC_MESSAGES)}
    finally:
        dist.destroy_process_group()


def sync_main():
    import os
    import torch.multiprocessing as mp
    world, port = 2, 29900 + os.getpid() % 2000
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_sync_worker, args=(r, world, port, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0, p.exitcode
    x, gy, convt, bn = _sync_case()
    convt, bn = convt.to(DEV).train(), bn.to(DEV).train()
    xd = x.to(DEV).requires_grad_()
    out = gnn.conv_transpose2x2_bn_gelu(xd, convt, bn)
    out.backward(gy.to(DEV))
    r0, r1 = ret[0], ret[1]

    def rel(a, b):
        return float((a - b.cpu()).norm() / b.cpu().norm().clamp_min(1e-12))
    res = {"out": rel(torch.cat([r0["out"], r1["out"]]), out.detach()), "dx": rel(torch.cat([r0["dx"], r1["dx"]]), xd.grad),
           "dw": rel(r0["dw"] + r1["dw"], convt.weight.grad), "dgamma": rel(r0["dgamma"] + r1["dgamma"], bn.weight.grad),
           "dbeta": rel(r0["dbeta"] + r1["dbeta"], bn.bias.grad), "running_mean": rel(r0["rm"], bn.running_mean),
           "running_var": rel(r0["rv"], bn.running_var), "running_mean_ranks": rel(r0["rm"], r1["rm"])}
    assert r0["nbt"] == r1["nbt"] == 1
    print(json.dumps({"rel_l2": res, "messages": [r0["msgs"], r1["msgs"]]}))


if __name__ == "__main__":
    {"graph": graph_main, "sync": sync_main}[sys.argv[1]]()
