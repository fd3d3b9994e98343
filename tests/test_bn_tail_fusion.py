"""Decoder tail without the normalised map (bf16 training): `fpn_bottleneck`'s BatchNorm + ReLU applied inside the classifier
head's kernels (gdl_head_1x1_bn) and the BatchNorm backward formed straight from the head's logit gradient
(gdl_bn_head_bwd_reduce / gdl_bn_head_bwd_dx), against the separate launches they replace (GDL_FUSE_BN_TAIL=0:
bn_apply -> head_1x1, head_1x1_bwd -> bn_bwd_reduce -> bn_bwd_dx) on the same inputs, and against torch f64 autograd.

The same for the laterals: their BatchNorm + ReLU applied to the base operand of the top-down add (gdl_bilinear_fwd_add_bn)
against bn_apply -> bilinear_add, factors 2 and 4, and the training node that owns a lateral and its add."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402

DEV = "cuda"
EPS = 1e-5
# the production shape in miniature, a ragged one (P % 16 == 9: the head's last 16-pixel tile is partial, and P % 8 != 0: the
# backward kernels' last row group is partial), and one whose pixel count gives both backward reductions 2048 partial rows
SHAPES = [(2, 144, 144, 5), (1, 67, 67, 5), (1, 67, 67, 3), (1, 67, 67, 8), (4, 384, 384, 5)]


def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)))


def _inputs(B, H, W, K, C=256):
    y = (_rnd(B, H, W, C) * 2 + 0.5).to(DEV, torch.bfloat16)
    g, b = _rnd(C, seed=1).to(DEV), _rnd(C, seed=2).to(DEV)
    w, bias = (_rnd(K, C, seed=3) * 0.1).to(DEV), _rnd(K, seed=4).to(DEV)
    dlow = (_rnd(B, H, W, K, seed=5) * 0.01).to(DEV)
    mean, var = ops.bn_stats(y)
    return y, g, b, w, bias, dlow, mean, var


def _unfused(y, g, b, w, bias, dlow, mean, var):
    P = y.numel() // y.shape[-1]
    z = ops.bn_apply(y, mean, var, g, b, EPS, True)
    low = ops.head_1x1(z, w, bias)
    dz, dw, db = ops.head_1x1_bwd(z, dlow, w, None)
    dg, dbt = ops.bn_bwd_reduce(y, dz, mean, var, g, b, EPS, True)
    dy = ops.bn_bwd_dx(y, dz, mean, var, g, b, EPS, True, dg, dbt, P)
    return low, dg, dbt, dw, db, dy


def _fused(y, g, b, w, bias, dlow, mean, var):
    P = y.numel() // y.shape[-1]
    low = ops.head_1x1_bn(y, mean, var, g, b, EPS, True, w, bias)
    dg, dbt, dw, db = ops.bn_head_bwd_reduce(y, dlow, w, mean, var, g, b, EPS, True)
    dy = ops.bn_head_bwd_dx(y, dlow, w, mean, var, g, b, EPS, True, dg, dbt, P)
    return low, dg, dbt, dw, db, dy


def _close(got, ref, tol, what, scale=None):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    s = ref.abs().max().item() if scale is None else scale
    err = (got - ref).abs().max().item()
    print(f"{what}: max err {err:.3e} (scale {s:.3e})")
    assert err <= tol * max(s, 1e-6), f"{what}: max err {err:.3e} vs scale {s:.3e}"


@pytest.mark.parametrize("B,H,W,K", SHAPES)
def test_fused_tail_matches_separate_kernels(B, H, W, K):
    """Forward: bit-identical logits (the same f32 expression and the one bf16 rounding of bn_apply, then the same MFMA head).
    dgamma / dbeta: bit-identical (the partial-row partition and the accumulation order of bn_bwd_partial8 are kept, dz is the
    bf16 value head_1x1_bwd writes).  Head dW / db: bit-identical where the head's own partition (P / 256 rows, at most 2048)
    equals BatchNorm's (P / 64, at most 2048), which the merged pass uses -- otherwise the f32 tolerance of test_batchnorm_train.
    dy: to one bf16 ulp, the bound test_head_mfma_and_register_weight_kernels uses for two kernels forming the same products."""
    inp = _inputs(B, H, W, K)
    low0, dg0, dbt0, dw0, db0, dy0 = _unfused(*inp)
    low1, dg1, dbt1, dw1, db1, dy1 = _fused(*inp)
    P = B * H * W
    print(f"P={P} K={K}: logits max diff {(low1 - low0).abs().max().item():.3e}, dgamma {(dg1 - dg0).abs().max().item():.3e}, "
          f"dbeta {(dbt1 - dbt0).abs().max().item():.3e}, dW {(dw1 - dw0).abs().max().item():.3e}, db {(db1 - db0).abs().max().item():.3e}, "
          f"dy {(dy1.float() - dy0.float()).abs().max().item():.3e} of {dy0.float().abs().max().item():.3e}")
    assert torch.equal(low1, low0), "head logits from the pre-BN map"
    assert torch.equal(dg1, dg0) and torch.equal(dbt1, dbt0), "dgamma / dbeta"
    if min(P // 256, 2048) == min(P // 64, 2048):
        assert torch.equal(dw1, dw0) and torch.equal(db1, db0), "head dW / db (same partial-row partition)"
    else:
        _close(dw1, dw0, 1e-4, "head dW")
        _close(db1, db0, 1e-4, "head db", scale=max(db0.abs().max().item(), 1e-3))
    assert (dy1.float() - dy0.float()).abs().max().item() <= 2.0 ** -7 * dy0.float().abs().max().item(), "dy"
    # in place over the saved convolution output, as the training node calls it
    y = inp[0].clone()
    out = ops.bn_head_bwd_dx(y, inp[5], inp[3], inp[6], inp[7], inp[1], inp[2], EPS, True, dg1, dbt1, P, out=y)
    assert out.data_ptr() == y.data_ptr() and torch.equal(y, dy1)


@pytest.mark.parametrize("relu", [True, False])
def test_fused_tail_without_bias_and_relu(relu):
    y, g, b, w, _, dlow, mean, var = _inputs(1, 67, 67, 5)
    z = ops.bn_apply(y, mean, var, g, b, EPS, relu)
    assert torch.equal(ops.head_1x1_bn(y, mean, var, g, b, EPS, relu, w, None), ops.head_1x1(z, w, None))
    dz, dw0, _ = ops.head_1x1_bwd(z, dlow, w, None)
    dg0, dbt0 = ops.bn_bwd_reduce(y, dz, mean, var, g, b, EPS, relu)
    dg1, dbt1, dw1, _ = ops.bn_head_bwd_reduce(y, dlow, w, mean, var, g, b, EPS, relu)
    assert torch.equal(dg1, dg0) and torch.equal(dbt1, dbt0)
    _close(dw1, dw0, 1e-4, "head dW")


@pytest.mark.parametrize("B,H,W,K", [(2, 144, 144, 5), (1, 67, 67, 5)])
def test_fused_tail_matches_torch_f64(B, H, W, K):
    """Independent reference: torch f64 autograd on the CPU for relu(batch_norm(y)) -> 1x1 conv, with the tolerance
    test_batchnorm_train gives a bf16 case (2e-2 of the largest reference value, for the maps and for the sums alike)."""
    y, g, b, w, bias, dlow, mean, var = _inputs(B, H, W, K)
    low, dg, dbt, dw, db, dy = _fused(y, g, b, w, bias, dlow, mean, var)
    yr = y.cpu().double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    gr, br = g.cpu().double().requires_grad_(True), b.cpu().double().requires_grad_(True)
    wr, biasr = w.cpu().double().requires_grad_(True), bias.cpu().double().requires_grad_(True)
    z = F.relu(F.batch_norm(yr, None, None, gr, br, True, 0.1, EPS))
    lr = F.conv2d(z, wr[:, :, None, None], biasr)
    lr.backward(dlow.cpu().double().permute(0, 3, 1, 2))
    bf = 2e-2
    _close(low.permute(0, 3, 1, 2), lr, bf, "logits vs f64")
    _close(dg, gr.grad, bf, "dgamma vs f64")
    _close(dbt, br.grad, bf, "dbeta vs f64")
    _close(dw, wr.grad, bf, "head dW vs f64")
    _close(db, biasr.grad, bf, "head db vs f64", scale=max(biasr.grad.abs().max().item(), 1e-3))
    _close(dy.permute(0, 3, 1, 2), yr.grad, bf, "dy vs f64", scale=yr.grad.abs().max().item() + 1e-3)


# ------------------------------------------------------------------------------------------------ top-down add
# (B, Ho, Wo, C, factor): the production shape in miniature; a ragged one (26 x 34 pixels: P % 16 == 4, an odd number of gaps per
# row); factor 4; a narrower map
ADD_SHAPES = [(2, 144, 144, 256, 2), (1, 34, 26, 256, 2), (2, 72, 72, 256, 4), (3, 20, 28, 64, 4)]


def _add_inputs(B, Ho, Wo, C, f):
    y = (_rnd(B, Ho, Wo, C) * 2 + 0.5).to(DEV, torch.bfloat16)
    up = _rnd(B, Ho // f, Wo // f, C, seed=6).to(DEV, torch.bfloat16)
    g, b = _rnd(C, seed=1).to(DEV), _rnd(C, seed=2).to(DEV)
    mean, var = ops.bn_stats(y)
    return y, up, g, b, mean, var


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("B,Ho,Wo,C,f", ADD_SHAPES)
def test_topdown_add_from_pre_bn_map_is_bit_identical(B, Ho, Wo, C, f, relu):
    """The top-down sum from the pre-BatchNorm lateral equals bn_apply followed by today's add kernel bit for bit (the base vector
    goes through bn_apply's f32 expression and one bf16 rounding before the add), and matches torch in f64 to the bf16 tolerance
    of test_batchnorm_train."""
    y, up, g, b, mean, var = _add_inputs(B, Ho, Wo, C, f)
    want = ops.bilinear_add(ops.bn_apply(y, mean, var, g, b, EPS, relu), up)
    got = ops.bilinear_add_bn(y, mean, var, g, b, EPS, relu, up)
    print(f"{(B, Ho, Wo, C)} x{f}: max diff {(got.float() - want.float()).abs().max().item():.3e}")
    assert torch.equal(got, want)
    z = F.batch_norm(y.cpu().double().permute(0, 3, 1, 2), None, None, g.cpu().double(), b.cpu().double(), True, 0.1, EPS)
    z = F.relu(z) if relu else z
    ref = z + F.interpolate(up.cpu().double().permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=False)
    _close(got.permute(0, 3, 1, 2), ref, 2e-2, "top-down sum vs f64")


@pytest.mark.parametrize("B,Ho,Wo,f", [(2, 48, 48, 2), (1, 34, 26, 2), (2, 48, 48, 4)])
def test_lateral_add_node_matches_separate_nodes(monkeypatch, B, Ho, Wo, f):
    """gnn.conv_bn_act_upsample_add (one node: 1x1 conv -> BN statistics -> add with BN + ReLU on load) against conv_bn_act ->
    upsample_add through the switch: the sum and every gradient are equal -- the forward is bit-identical and the backward
    launches the same kernels on the same operands."""
    from geo_deep_learning.models.utils import ConvModule
    cin, C = 128, 256
    mod = ConvModule(cin, C, 1, inplace=False).to(DEV).train()
    with torch.no_grad():
        mod.norm.weight.copy_(_rnd(C, seed=1).abs() + 0.5)
        mod.norm.bias.copy_(_rnd(C, seed=2) * 0.2)
    x0 = _rnd(B, Ho, Wo, cin).to(DEV, torch.bfloat16)
    up0 = _rnd(B, Ho // f, Wo // f, C, seed=6).to(DEV, torch.bfloat16)
    gout = _rnd(B, Ho, Wo, C, seed=7).to(DEV, torch.bfloat16)
    calls = [0]
    real = ops.bilinear_add_bn

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, "bilinear_add_bn", counted)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(gnn, "FUSE_BN_TAIL", on)
        mod.zero_grad(set_to_none=True)
        rm, rv = mod.norm.running_mean.clone(), mod.norm.running_var.clone()
        x, up = x0.clone().requires_grad_(True), up0.clone().requires_grad_(True)
        before = calls[0]
        out = gnn.conv_bn_act_upsample_add(x, mod.conv, mod.norm, up)
        assert (calls[0] - before == 1) == on, "the switch selects the fused node"
        out.backward(gout)
        res[on] = dict(out=out.detach(), dx=x.grad, dup=up.grad, dw=mod.conv.weight.grad.clone(), dgamma=mod.norm.weight.grad.clone(),
                       dbeta=mod.norm.bias.grad.clone(), rm=mod.norm.running_mean.clone(), rv=mod.norm.running_var.clone())
        with torch.no_grad():
            mod.norm.running_mean.copy_(rm)
            mod.norm.running_var.copy_(rv)
    for k in res[True]:
        d = (res[True][k].float() - res[False][k].float()).abs().max().item()
        print(f"{k}: max diff {d:.3e}")
        assert torch.equal(res[True][k], res[False][k]), k


def test_head_on_materialised_map_when_the_concat_node_does_not_apply(monkeypatch):
    """concat_resize_conv_bn_act(head_conv=...) where the fused training node is not available (here: FUSE_CONCAT_BWD off): the head
    runs on the materialised ConvModule output and gives the logits of the two separate calls."""
    import copy
    from geo_deep_learning.models.utils import ConvModule
    mod = ConvModule(512, 256, 3, padding=1, inplace=True).to(DEV).train()
    head = torch.nn.Conv2d(256, 5, 1).to(DEV)
    levels = [_rnd(2, 48, 48, 256).to(DEV, torch.bfloat16), _rnd(2, 24, 24, 256, seed=1).to(DEV, torch.bfloat16)]
    monkeypatch.setattr(gnn, "FUSE_CONCAT_BWD", False)
    norm2 = copy.deepcopy(mod.norm)
    low = gnn.concat_resize_conv_bn_act(levels, mod.conv, mod.norm, head_conv=head)
    dec = gnn.concat_resize_conv_bn_act(levels, mod.conv, norm2)
    want = ops.head_1x1(dec, head.weight.detach(), head.bias.detach())
    assert low.shape == (2, 48, 48, 5) and torch.equal(low, want)


def test_dofa_training_step_switch_on_and_off(monkeypatch):
    """One SegmentationDOFA training step (bf16 autocast, tiny encoder, nothing frozen, decoder map 4 x 32 x 32 x 256) with the
    switch on and one with it off, from the same parameters and the same device-RNG seed.  The loss is equal (bit-identical
    logits and top-down sums).  Gradients: equal, for every parameter but the head's weight and bias -- dy, dgamma and dbeta of the
    fused tail are bit-identical to the separate kernels' at every shape measured (test_fused_tail_matches_separate_kernels), the
    laterals' backward launches the same kernels on the same operands, and everything upstream is a function of those.  The head's
    dW / db are summed over P / 64 partial rows instead of P / 256: f32 tolerance of test_batchnorm_train (largest difference seen:
    4e-8 of the gradient's norm)."""
    from test_hip_tasks import _Trainer, _dofa_task, _to_dev, synthetic_batch
    b, nc = 4, 5
    batch = synthetic_batch(b, 3, 112, nc, 7)
    batch["wavelengths"] = batch["wavelengths"].unsqueeze(0).expand(b, -1).contiguous()
    dev = _to_dev(batch)
    calls = {"head_1x1_bn": 0, "bilinear_add_bn": 0}
    for name in calls:
        def counted(*a, _real=getattr(ops, name), _name=name, **k):
            calls[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(gnn, "FUSE_BN_TAIL", on)
        _, task = _dofa_task(freeze=None)
        task.trainer = _Trainer(True)
        task.train()
        torch.manual_seed(123)
        before = dict(calls)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = task.training_step(dev, 0)
        loss.backward()
        assert calls["head_1x1_bn"] - before["head_1x1_bn"] == (1 if on else 0), "the switch selects the fused tail"
        assert calls["bilinear_add_bn"] - before["bilinear_add_bn"] == (3 if on else 0), "the switch selects the fused lateral adds"
        res[on] = (loss.item(), {n: p.grad.detach().float().clone() for n, p in task.model.named_parameters() if p.grad is not None})
    (l1, g1), (l0, g0) = res[True], res[False]
    assert g1.keys() == g0.keys() and len(g1) > 100
    worst, wname = 0.0, ""
    for n in g0:
        err, rn = (g1[n] - g0[n]).norm().item(), g0[n].norm().item()
        if rn > 0 and err / rn > worst:
            worst, wname = err / rn, n
    print(f"loss {l1!r} (fused) vs {l0!r}; largest relative gradient difference {worst:.3e} ({wname})")
    assert l1 == l0
    reordered = ("head.conv.weight", "head.conv.bias")
    for n in g0:
        if n in reordered:
            _close(g1[n], g0[n], 1e-4, n, scale=max(g0[n].abs().max().item(), 1e-3))
        else:
            assert torch.equal(g1[n], g0[n]), (n, (g1[n] - g0[n]).abs().max().item(), g0[n].abs().max().item())
