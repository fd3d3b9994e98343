"""GPU tests of the UperNet scale_modules path (reference upernet.py:37-54,113-119): ConvTranspose2d(2, 2), BatchNorm -> GELU and
the 2x2 max-pool as HIP kernels.  Operator level against torch on the CPU (f32 autograd on the same -- for bf16: the bf16-rounded
-- inputs), decoder level against the golden of the real reference (tools/make_golden_scale_modules.py).

Bounds (the project's existing ones, tests/test_hip_ops.py "production shape" node tests): f32 within 2e-5 relative L2, bf16 within
6e-3 relative L2 of f32 torch on the bf16-rounded inputs.  Every test prints what it measured before it asserts."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402
from geo_deep_learning.models.decoders.upernet import UperNetDecoder  # noqa: E402
from oracle import procedural_state_dict  # noqa: E402

from _scale_modules_recipe import load_golden, recipe_inputs  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
BOUND = {torch.float32: 2e-5, torch.bfloat16: 6e-3}
HERE = Path(__file__).resolve().parent


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g)


def q(t, dtype):
    """The value the device sees: rounded to the compute dtype, as f32."""
    return t.to(dtype).float()


def rel_l2(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-12))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def cl(g):
    """Cotangent on the device in the layout of the decoder's output (channels last), as a loss behind the heads delivers it."""
    return g.to(DEV).contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------ 3. ConvTranspose2d(2, 2)
CONVT_CASES = {"toy": (2, 5, 7, 16, 24, False), "sliced": (2, 6, 4, 32, 16, True), "fpn1.0": (4, 36, 36, 768, 384, False),
               "fpn1.3": (4, 72, 72, 384, 192, False)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", list(CONVT_CASES))
def test_conv_transpose2x2_against_torch(case, dtype):
    """Forward / data gradient / weight gradient / bias gradient of the autograd node against F.conv_transpose2d on the CPU.
    Measured (MI355X): f32 <= 5.1e-6 (the bias gradient's column sum at 72^2 x 4 pixels; GEMMs <= 9.8e-7), bf16 <= 1.71e-3
    (output and dx: their own bf16 rounding; dw / db are f32 outputs, <= 5e-7)."""
    B, H, W, cin, cout, sliced = CONVT_CASES[case]
    x = q(rnd(B, cin, H, W, seed=1), dtype)
    convt = nn.ConvTranspose2d(cin, cout, 2, 2)
    with torch.no_grad():
        convt.weight.copy_(q(rnd(cin, cout, 2, 2, seed=2) * (2.0 / cin) ** 0.5, dtype))
        convt.bias.copy_(rnd(cout, seed=3) * 0.1)
    gy = q(rnd(B, cout, 2 * H, 2 * W, seed=4), dtype)
    xr = x.clone().requires_grad_()
    ref = F.conv_transpose2d(xr, convt.weight, convt.bias, stride=2)
    ref.backward(gy)
    want = {"out": ref.detach(), "dx": xr.grad, "dw": convt.weight.grad.clone(), "db": convt.bias.grad.clone()}
    convt.zero_grad()
    convt = convt.to(DEV).train()
    if sliced:      # a channel slice of a wider buffer: strided pixels
        buf = torch.zeros(B, H, W, cin + 16, device=DEV, dtype=dtype)
        buf[..., 8:8 + cin] = nhwc(x).to(DEV, dtype)
        xd = buf[..., 8:8 + cin].requires_grad_()
    else:
        xd = nhwc(x).to(DEV, dtype).requires_grad_()
    out = gnn.conv_transpose2x2(xd, convt)
    out.backward(nhwc(gy).to(DEV, dtype))
    got = {"out": nchw(out), "dx": nchw(xd.grad), "dw": convt.weight.grad, "db": convt.bias.grad}
    assert convt.weight.grad.shape == convt.weight.shape and convt.weight.grad.is_contiguous()
    res = {k: rel_l2(got[k], want[k]) for k in want}
    print(f"convT {case} {dtype}: " + ", ".join(f"{k} {v:.2e}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not v <= BOUND[dtype]}
    assert not bad, bad


def test_convt_wgrad_accumulates_and_channel_constraint_is_a_value_error():
    x, dy = rnd(1, 4, 4, 8, seed=5).to(DEV), rnd(1, 8, 8, 8, seed=6).to(DEV)
    once = ops.convt2x2_wgrad(x, dy)
    twice = ops.convt2x2_wgrad(x, dy, out=once.clone(), accumulate=True)
    assert torch.equal(twice, once + once)
    with pytest.raises(ValueError, match="multiples of 8"):
        ops.convt2x2_pack(torch.zeros(12, 8, 2, 2, device=DEV), torch.bfloat16)
    with pytest.raises(ValueError, match="multiples of 4"):
        ops.convt2x2_pack(torch.zeros(8, 6, 2, 2, device=DEV), torch.float32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.maxpool2x2s2(torch.zeros(1, 4, 4, 8))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.bn_gelu_apply(torch.zeros(4, 8), torch.zeros(8), torch.ones(8), torch.ones(8), torch.zeros(8), 1e-5)


# ------------------------------------------------------------------ 4. ConvTranspose -> BatchNorm -> GELU
BNG_CASES = {"toy": (2, 5, 7, 16, 24), "tail": (1, 3, 11, 8, 40), "fpn1": (4, 36, 36, 768, 384)}


def _bn_gelu_case(case, dtype, seed=10):
    B, H, W, cin, cout = BNG_CASES[case]
    x = q(rnd(B, cin, H, W, seed=seed), dtype)
    convt, bn = nn.ConvTranspose2d(cin, cout, 2, 2), nn.BatchNorm2d(cout)
    with torch.no_grad():
        convt.weight.copy_(q(rnd(cin, cout, 2, 2, seed=seed + 1) * (2.0 / cin) ** 0.5, dtype))
        convt.bias.copy_(rnd(cout, seed=seed + 2) * 0.1)
        bn.weight.copy_(1 + 0.2 * rnd(cout, seed=seed + 3))
        bn.bias.copy_(0.3 * rnd(cout, seed=seed + 4))
        bn.running_mean.copy_(0.1 * rnd(cout, seed=seed + 5))
        bn.running_var.copy_(1 + 0.3 * rnd(cout, seed=seed + 6).abs())
    gy = q(rnd(B, cout, 2 * H, 2 * W, seed=seed + 7), dtype)
    return x, convt, bn, gy


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", list(BNG_CASES))
def test_conv_transpose_bn_gelu_train_node_against_torch(case, dtype):
    """Train mode: output, running statistics (momentum 0.1), num_batches_tracked, dx, dw, dgamma, dbeta against
    F.gelu(F.batch_norm(F.conv_transpose2d(.))) autograd on the CPU; "tail": 33 x 4 = 132 pixels, not a multiple of the
    kernels' pixel rows per step (256 / (C / V) = 25 at C = 40 f32, 51 for bf16).
    Measured (MI355X): f32 <= 9.9e-7 for every tensor; bf16 out <= 2.49e-3, dx <= 2.43e-3, dw <= 1.98e-3, dgamma <= 1.89e-3,
    dbeta <= 6.7e-4, running statistics <= 2.1e-4."""
    import copy
    x, convt, bn, gy = _bn_gelu_case(case, dtype)
    ct, bt = copy.deepcopy(convt), copy.deepcopy(bn).train()
    xr = x.clone().requires_grad_()
    ref = F.gelu(bt(ct(xr)))
    ref.backward(gy)
    want = {"out": ref.detach(), "dx": xr.grad, "dw": ct.weight.grad, "dgamma": bt.weight.grad, "dbeta": bt.bias.grad,
            "running_mean": bt.running_mean, "running_var": bt.running_var}
    convt, bn = convt.to(DEV).train(), bn.to(DEV).train()
    xd = nhwc(x).to(DEV, dtype).requires_grad_()
    out = gnn.conv_transpose2x2_bn_gelu(xd, convt, bn)
    out.backward(nhwc(gy).to(DEV, dtype))
    got = {"out": nchw(out), "dx": nchw(xd.grad), "dw": convt.weight.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
           "running_mean": bn.running_mean, "running_var": bn.running_var}
    res = {k: rel_l2(got[k], want[k]) for k in want}
    print(f"convT-BN-GELU {case} {dtype}: " + ", ".join(f"{k} {v:.2e}" for k, v in res.items()),
          f"| d bias {convt.bias.grad.abs().max().item():.1e}")
    assert int(bn.num_batches_tracked) == 1 == int(bt.num_batches_tracked)
    assert convt.bias.grad.abs().max().item() == 0.0          # analytically zero in front of a train-mode BatchNorm
    bad = {k: v for k, v in res.items() if not v <= BOUND[dtype]}
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_conv_transpose_bn_gelu_eval(dtype):
    x, convt, bn, _ = _bn_gelu_case("toy", dtype, seed=30)
    bn.eval()
    with torch.no_grad():
        want = F.gelu(bn(convt(x)))
    convt, bn = convt.to(DEV).eval(), bn.to(DEV).eval()
    xd = nhwc(x).to(DEV, dtype)
    with torch.no_grad():
        got = gnn.conv_transpose2x2_bn_gelu(xd, convt, bn)
    err = rel_l2(nchw(got), want)
    print(f"convT-BN-GELU eval {dtype}: {err:.2e}")
    assert err <= BOUND[dtype]
    with pytest.raises(NotImplementedError, match="eval-mode BatchNorm"):
        gnn.conv_transpose2x2_bn_gelu(xd.clone().requires_grad_(), convt, bn)


# ------------------------------------------------------------------ 5. MaxPool2d(2, 2)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H,W,C", [(2, 16, 16, 64), (1, 7, 7, 8), (2, 9, 12, 24), (4, 36, 36, 768)])
def test_maxpool2x2(dtype, B, H, W, C):
    """Forward bit-equal to torch; backward bit-equal in f32, within 2e-2 * max|dy| in bf16 (the 3x3 test's rule); planted ties
    (post-ReLU zeros, rounded values) and odd maps whose last row / column is dropped and gets zero gradient."""
    x = rnd(B, H, W, C).to(dtype).float()
    x[0, :6, :6] = x[0, :6, :6].clamp_min(0).round()
    xr = x.clone().requires_grad_()
    y = F.max_pool2d(xr.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    dy = rnd(*y.shape, seed=1).to(dtype).float()
    y.backward(dy)
    xd = x.to(DEV, dtype).requires_grad_()
    yd = gnn.maxpool2x2(xd)
    assert yd.shape == y.shape and torch.equal(yd.float().cpu(), y.detach())
    yd.backward(dy.to(DEV, dtype))
    dx = xd.grad.float().cpu()
    err = (dx - xr.grad).abs().max().item()
    print(f"maxpool2x2 {dtype} {(B, H, W, C)}: dx max err {err:.2e}")
    if dtype == torch.float32:
        assert torch.equal(dx, xr.grad)
    else:
        assert err <= 2e-2 * dy.abs().max().item()
    if H % 2:
        assert dx[:, H - 1].abs().max().item() == 0.0
    if W % 2:
        assert dx[:, :, W - 1].abs().max().item() == 0.0


# ------------------------------------------------------------------ 7 / 8. decoder against the golden of the real reference
def _decoder(meta, dtype_dev=DEV):
    dec = UperNetDecoder([meta["embed"]] * 4, channels=meta["channels"], align_corners=False, scale_modules=True)
    dec.load_state_dict(procedural_state_dict(dec, meta["seed"]))
    return dec.to(dtype_dev)


def _grad_rule(name, got, ref):
    """tests/test_hip_model.py:70-82 with rel = 2e-2: norm within 2e-2 (+ 2e-5), at most 1 % of the elements off by more than
    5 * rel * max|ref| (here: every element, not a sample)."""
    got, ref = got.detach().double().cpu(), torch.from_numpy(np.asarray(ref)).double()
    gn, rn = got.norm().item(), ref.norm().item()
    bad = ((got - ref).abs() > 5 * 2e-2 * ref.abs().max() + 1e-9).double().mean().item()
    print(f"  grad {name}: norm {gn:.6e} vs {rn:.6e}, rel l2 {((got - ref).norm() / max(rn, 1e-30)).item():.2e}, share off {bad:.4f}")
    return abs(gn - rn) <= 2e-2 * rn + 2e-5 and bad <= 0.01


def _run_decoder_train(dec, xs, g, dtype):
    hooks = {}
    xd = [x.to(DEV).requires_grad_() for x in xs]
    orig = dec.scale_inputs_nhwc
    dec.scale_inputs_nhwc = lambda inputs: hooks.setdefault("scaled", orig(inputs))
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            out = dec(xd)
        (out.float() * cl(g)).sum().backward()
    finally:
        del dec.scale_inputs_nhwc
    return out, hooks["scaled"], xd


def test_decoder_f32_against_reference_golden():
    """f32 decoder, train-mode forward + backward and eval forward, against the REAL reference's values.  Values within
    1e-3 * max|golden| (every element); gradients by _grad_rule; the three ConvTranspose biases feed a train-mode BatchNorm
    (fpn1.0.bias directly, fpn1.3.bias / fpn2.0.bias through the lateral 1x1 convolution): analytically zero, <= 1e-6 on both
    sides.  The reference compared with itself in float64 leaves 0 % of the elements off (meta f64_worst_share_off).
    Measured (MI355X): fpn1 / fpn2 / running statistics / eval fpn1 <= 2.7e-7 of max|golden|, fpn4 exact, train output 1.49e-4,
    eval output 3.4e-6; gradients: norms within 2.4e-3, relative L2 5.5e-3 .. 9.8e-3, 0 % of the elements off; zero-gradient
    biases 0 / 1.2e-7 / 7.7e-8 (reference 9.6e-8 / 5.6e-7 / 1.3e-7)."""
    gold, meta = load_golden()
    xs, g = recipe_inputs(meta)
    dec = _decoder(meta).train()
    out, scaled, xd = _run_decoder_train(dec, xs, g, torch.float32)
    vals = {"train_fpn1": nchw(scaled[0]), "train_fpn2": nchw(scaled[1]), "train_fpn4": nchw(scaled[3]), "train_out": out,
            "running_mean": dec.fpn1[1].running_mean, "running_var": dec.fpn1[1].running_var}
    ok = True
    for k, v in vals.items():
        ref = torch.from_numpy(gold[k])
        err, scale = (v.detach().float().cpu() - ref).abs().max().item(), ref.abs().max().item()
        print(f"  {k}: max err {err:.3e} / max|golden| {scale:.3e} = {err / scale:.2e}")
        ok &= err <= 1e-3 * scale
    assert int(dec.fpn1[1].num_batches_tracked) == 1
    params = dict(dec.named_parameters())
    for i in range(4):
        ok &= _grad_rule(f"input{i}", xd[i].grad, gold[f"grad_input{i}"])
    for n in meta["fpn_params"]:
        if n in meta["zero_grad"]:
            a, b = params[n].grad.double().norm().item(), float(np.linalg.norm(gold["grad/" + n].astype(np.float64)))
            print(f"  grad {n} (analytically zero): {a:.2e} vs reference {b:.2e}")
            ok &= a <= 1e-6 and b <= 1e-6
        else:
            ok &= _grad_rule(n, params[n].grad, gold["grad/" + n])
    dec.eval()
    st = meta["eval_stride"]
    with torch.no_grad():
        ev = {"eval_fpn1_s": nchw(dec.scale_inputs_nhwc([ops.as_nhwc(x.to(DEV)) for x in xs])[0])[:, :, 1::st, 1::st],
              "eval_out_s": dec([x.to(DEV) for x in xs])[:, :, 1::st, 1::st]}
    for k, v in ev.items():
        ref = torch.from_numpy(gold[k])
        err, scale = (v.float().cpu() - ref).abs().max().item(), ref.abs().max().item()
        print(f"  {k}: max err {err:.3e} / max|golden| {scale:.3e} = {err / scale:.2e}")
        ok &= err <= 1e-3 * scale
    assert ok


class _TorchDecoder(nn.Module):
    """The reference graph (upernet.py:111-152) spelled with torch.nn functions over the build's own parameter containers: what
    torch itself computes for this module, for the bf16-autocast yardstick."""

    def __init__(self, dec):
        super().__init__()
        self.d = dec

    @staticmethod
    def cm(m, x):
        x = F.conv2d(x, m.conv.weight, m.conv.bias, padding=m.conv.padding)
        x = F.batch_norm(x, m.norm.running_mean, m.norm.running_var, m.norm.weight, m.norm.bias, m.norm.training, 0.1, m.norm.eps)
        return F.relu(x) if m.act is not None else x

    def forward(self, inputs):
        d = self.d
        f1 = d.fpn1
        h = F.conv_transpose2d(inputs[0], f1[0].weight, f1[0].bias, stride=2)
        h = F.gelu(F.batch_norm(h, f1[1].running_mean, f1[1].running_var, f1[1].weight, f1[1].bias, f1[1].training, 0.1, f1[1].eps))
        ins = [F.conv_transpose2d(h, f1[3].weight, f1[3].bias, stride=2),
               F.conv_transpose2d(inputs[1], d.fpn2[0].weight, d.fpn2[0].bias, stride=2), inputs[2], F.max_pool2d(inputs[3], 2, 2)]
        lats = [self.cm(m, ins[i]) for i, m in enumerate(d.lateral_convs)]
        x = ins[-1]
        psp = [x]
        for ppm in d.psp_modules:
            p = self.cm(ppm[1], F.adaptive_avg_pool2d(x, ppm[0].output_size))
            psp.append(F.interpolate(p, size=x.shape[2:], mode="bilinear", align_corners=False))
        lats.append(self.cm(d.bottleneck, torch.cat(psp, 1)))
        for i in range(len(lats) - 1, 0, -1):
            lats[i - 1] = lats[i - 1] + F.interpolate(lats[i], size=lats[i - 1].shape[2:], mode="bilinear", align_corners=False)
        outs = [self.cm(d.fpn_convs[i], lats[i]) for i in range(len(lats) - 1)] + [lats[-1]]
        outs = [outs[0]] + [F.interpolate(o, size=outs[0].shape[2:], mode="bilinear", align_corners=False) for o in outs[1:]]
        return self.cm(d.fpn_bottleneck, torch.cat(outs, 1))


def test_decoder_bf16_no_worse_than_torch_autocast():
    """bf16 (autocast) decoder, train-mode forward, against the f32 golden, relative to torch's own bf16 autocast of the same
    graph on the CPU (tests/test_hip_model.py:345-373): max and RMS error <= 1.25 x torch's.  The f32 run of the torch graph must
    itself reproduce the golden (it is the reference graph).
    Measured (MI355X): build max 9.05e-2 rms 1.07e-2; torch autocast max 1.135e-1 rms 1.48e-2."""
    import copy
    gold, meta = load_golden()
    xs, g = recipe_inputs(meta)
    want = torch.from_numpy(gold["train_out"])
    tdec = _TorchDecoder(_decoder(meta, "cpu").train())
    with torch.no_grad():
        t32 = copy.deepcopy(tdec)(xs)
        assert (t32 - want).abs().max().item() <= 1e-4 * want.abs().max().item()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            theirs = copy.deepcopy(tdec)(xs).float()
    dec = _decoder(meta).train()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ours = dec([x.to(DEV) for x in xs]).float().cpu()
    e_o, e_t = ours - want, theirs - want
    mx = (e_o.abs().max().item(), e_t.abs().max().item())
    rms = (e_o.pow(2).mean().sqrt().item(), e_t.pow(2).mean().sqrt().item())
    print(f"bf16 decoder vs f32 golden -- build: max {mx[0]:.3e} rms {rms[0]:.3e}; torch autocast: max {mx[1]:.3e} rms {rms[1]:.3e}")
    assert mx[0] <= 1.25 * mx[1] and rms[0] <= 1.25 * rms[1], (mx, rms)


# ------------------------------------------------------------------ 9. operand freshness
def _two_steps(meta, xs, g, clear_cache):
    torch.manual_seed(5)
    dec = _decoder(meta).train()
    opt = gnn.FusedAdam([p for p in dec.parameters()], lr=1e-2)
    outs = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = dec([x.to(DEV) for x in xs])
        (out.float() * cl(g)).sum().backward()
        opt.step()
        outs.append(out.detach().float().cpu())
        if clear_cache:
            gnn._CACHE.clear()
    return outs


def test_second_bf16_step_uses_the_updated_conv_transpose_weights():
    """Two bf16 training steps with FusedAdam: the second step's output is bit-equal to a run in which every cached operand is
    dropped between the steps, and differs from the first step's (the update was seen)."""
    _, meta = load_golden()
    xs, g = recipe_inputs(meta)
    g = g * 512          # a gradient large enough that one Adam step moves bf16 operands
    a, b = _two_steps(meta, xs, g, False), _two_steps(meta, xs, g, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], a[1])


def test_captured_step_replays_match_eager_steps():
    """forward + backward + FusedAdam.step of the decoder under torch.cuda.graph, in its own process: three replays bit-equal to
    three eager steps (tests/_scale_modules_worker.py)."""
    r = subprocess.run([sys.executable, str(HERE / "_scale_modules_worker.py"), "graph"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["replays"] == 3 and res["outputs_equal"] == [True, True, True] and res["params_equal"] and res["moved"]


# ------------------------------------------------------------------ 6. SyncBatchNorm at world size 2 on one GPU
def test_syncbn_world2_on_one_gpu_matches_full_batch():
    """Two processes (gloo on device tensors) run the ConvTranspose -> SyncBatchNorm -> GELU node on half the batch each; the
    concatenated outputs / input gradients, the summed parameter gradients and the running statistics must equal the one-process
    full-batch result (same kernels; the statistics are merged in another order: 2e-5 relative L2, f32)."""
    r = subprocess.run([sys.executable, str(HERE / "_scale_modules_worker.py"), "sync"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["messages"] == [[1, 1], [1, 1]]
    bad = {k: v for k, v in res["rel_l2"].items() if not v <= 2e-5}
    assert not bad, bad


# ------------------------------------------------------------------ 10. frozen parts
def test_frozen_fpn1_computes_no_weight_gradients(monkeypatch):
    _, meta = load_golden()
    xs, g = recipe_inputs(meta)
    dec = _decoder(meta).train()
    for p in dec.fpn1.parameters():
        p.requires_grad_(False)
    calls = {"wgrad": 0, "pack": 0}
    real_w, real_p = ops.convt2x2_wgrad, ops.convt2x2_pack
    monkeypatch.setattr(ops, "convt2x2_wgrad", lambda *a, **k: (calls.__setitem__("wgrad", calls["wgrad"] + 1), real_w(*a, **k))[1])
    monkeypatch.setattr(ops, "convt2x2_pack", lambda *a, **k: (calls.__setitem__("pack", calls["pack"] + 1), real_p(*a, **k))[1])
    xd = [x.to(DEV).requires_grad_() for x in xs]
    for _ in range(2):
        out = dec(xd)
        (out * cl(g)).sum().backward()
    assert all(x.grad is not None and x.grad.abs().max().item() > 0 for x in xd)
    assert all(p.grad is None for p in dec.fpn1.parameters())
    assert dec.fpn2[0].weight.grad is not None and dec.fpn2[0].bias.grad is not None
    # per step: one weight gradient (fpn2.0 only); packs: fpn2.0 in every forward (trained), the two frozen fpn1 weights once
    assert calls == {"wgrad": 2, "pack": 2 + 2}, calls
