"""gdlhip.nn.LovaszLoss on the GPU: the segmented radix sort (gdl_sort_desc_f32) against torch.sort on the CPU, exactly; the
gdl_lovasz_* kernels in multiclass and binary mode, forward and backward with the auxiliary head's upstream factor, against
``lovasz_ref`` (tests/test_lovasz_host.py: the definition restated with torch, here in f64); edge semantics, determinism, plumbing
and a captured training step.

Tolerances are measured, not guessed: the same restatement run in f32 on the CPU deviates from f64 by at most the MEASURED_*
figures below over the cases of this file (``python tests/test_lovasz_host.py`` prints them: loss absolute, gradient relative to
the largest gradient element); the kernels get 4x that -- a different but equally valid f32 summation order and near-tie rank
swaps.  No element is excluded from a comparison."""

import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_for_lovasz", Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


H = _load("test_lovasz_host")
rnd, make_target = H.rnd, H.make_target

DEV = "cuda"
UP = 0.4          # the upstream factor of the auxiliary head
T = H.SORT_TILE

# f32-vs-f64 deviation of lovasz_ref on the CPU, maximum over MULTICLASS_CASES / BINARY_CASES (the loss of most cases reads about
# 3e-8, the gradient about 6e-7 of its largest element; the maxima come from single near-tie rank swaps)
MEASURED_LOSS_DEV = {"multiclass": 8.575e-08, "binary": 2.384e-07}
MEASURED_GRAD_DEV = {"multiclass": 4.361e-04, "binary": 1.072e-04}
LOSS_TOL = {m: 4 * v for m, v in MEASURED_LOSS_DEV.items()}
GRAD_TOL = {m: 4 * v for m, v in MEASURED_GRAD_DEV.items()}


def check_case(mode, shape, ignore, per_image, extra):
    """LovaszLoss(mode, per_image, ignore) on a case of tests/test_lovasz_host.py against its shared f64 reference."""
    logits, y = H.multiclass_case(shape, ignore, extra) if mode == "multiclass" else H.binary_case(shape, ignore, extra)
    ref, gref = H.reference(mode, shape, ignore, per_image, extra, torch.float64, UP)
    ld = logits.to(DEV).requires_grad_(True)
    loss = gnn.LovaszLoss(mode, per_image=per_image, ignore_index=ignore)(ld, y.to(DEV))
    (UP * loss).backward()
    grad = ld.grad.cpu()
    assert loss.dim() == 0 and torch.isfinite(loss).item() and torch.isfinite(grad).all().item()
    what = f"{mode} {shape} ignore={ignore} per_image={per_image} {extra}"
    err = abs(loss.item() - ref.item())
    scale = gref.abs().max().item()
    gerr = (grad.double() - gref).abs().max().item()
    print(f"{what}: loss {loss.item():.8f} ref {ref.item():.8f} err {err:.3e} bound {LOSS_TOL[mode]:.3e}; "
          f"grad max err {gerr:.3e} = {gerr / max(scale, 1e-300):.3e} of the scale {scale:.3e}, bound {GRAD_TOL[mode]:.3e}")
    assert err <= LOSS_TOL[mode], what
    assert gerr <= GRAD_TOL[mode] * scale, what
    if ignore is not None:
        gi = grad.reshape(shape[0], shape[1], -1).permute(0, 2, 1)[(y == ignore).reshape(shape[0], -1)]
        assert gi.numel() > 0 and (gi == 0).all(), "the gradient of an ignored pixel is exactly 0 in every class"
    return loss, grad


# ------------------------------------------------------------------------------------------------ 1. the sort, exact
def _from_bits(bits):
    return bits.to(torch.int32).view(torch.float32)


def key_set(kind, S, n, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        return torch.rand(S, n, generator=g)
    if kind == "four_values":
        return torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (S, n), generator=g)]
    if kind == "lowest_digit":
        return _from_bits(0x3F000000 + torch.randint(0, 256, (S, n), generator=g))
    if kind == "highest_digit":
        return _from_bits(torch.randint(0, 128, (S, n), generator=g) << 24)
    if kind == "zeros":
        return torch.zeros(S, n)
    assert kind == "zeros_and_denormals"
    bits = torch.randint(1, 1 << 23, (S, n), generator=g)
    return _from_bits(torch.where(torch.rand(S, n, generator=g) < 0.5, torch.zeros_like(bits), bits))


# T - 1, T, T + 1: around one tile; 3T + 17: a ragged last tile; 8T + 1: the first length whose (digit, workgroup) table no
# longer fits one scan workgroup (reduce / spine / apply instead of apply alone)
SORT_LENGTHS = (1, 2, T - 1, T, T + 1, 3 * T + 17, H.MULTI_SCAN_N, H.MULTI_SCAN_N + 1)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("kind", ["uniform", "four_values", "lowest_digit", "highest_digit", "zeros", "zeros_and_denormals"])
def test_sort_equals_torch_stable_descending_sort(kind, S):
    assert H.MULTI_SCAN_N == 8 * T + 1 and 256 * 8 == H.SCAN_TABLE_TILE
    for n in SORT_LENGTHS:
        keys = key_set(kind, S, n, seed=n + S)
        assert (keys >= 0).all() and torch.isfinite(keys).all()
        want, want_perm = torch.sort(keys, dim=1, descending=True, stable=True)
        got, perm = ops.sort_desc_f32(keys.to(DEV))
        assert perm.dtype == torch.int32 and got.shape == keys.shape
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), (kind, S, n, "keys")
        assert torch.equal(perm.cpu().long(), want_perm), (kind, S, n, "permutation")


# ------------------------------------------------------------------------------------------------ 2./3. multiclass
@pytest.mark.parametrize("shape,ignore,per_image,std", H.MULTICLASS_CASES)
def test_multiclass(shape, ignore, per_image, std):
    check_case("multiclass", shape, ignore, per_image, std)


def test_unsqueezed_mask_bf16_and_strided_logits_equal_the_plain_call():
    shape = (2, 5, 24, 40)
    logits, y = H.multiclass_case(shape, 255, 2.0)
    crit = gnn.LovaszLoss("multiclass", ignore_index=255)
    xd, yd = logits.to(DEV), y.to(DEV)
    base = crit(xd, yd)
    assert torch.equal(crit(xd, yd[:, None]), base)
    nhwc = xd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # same values, other strides
    assert not nhwc.is_contiguous() and torch.equal(crit(nhwc, yd), base)
    xb = xd.to(torch.bfloat16).requires_grad_(True)
    xf = xb.detach().float().requires_grad_(True)
    lb, lf = crit(xb, yd), crit(xf, yd)
    lb.backward()
    lf.backward()
    assert torch.equal(lb, lf) and xb.grad.dtype == torch.bfloat16 and torch.equal(xb.grad, xf.grad.to(torch.bfloat16))


def test_lowres_logits_are_materialised():
    low = (rnd(2, 9, 11, 5, seed=3) * 2.0).to(DEV)
    y = make_target((2, 24, 40), 5, 255, seed=4).to(DEV)
    crit = gnn.LovaszLoss("multiclass", ignore_index=255)
    a = low.clone().requires_grad_(True)
    la = crit(gnn.LowresLogits(a, (24, 40)), y)
    la.backward()
    b = low.clone().requires_grad_(True)
    lb = crit(gnn.LowresLogits(b, (24, 40)).materialise(), y)
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad) and a.grad.abs().max().item() > 0


# ------------------------------------------------------------------------------------------------ 4. binary
@pytest.mark.parametrize("shape,ignore,per_image,kind", H.BINARY_CASES)
def test_binary(shape, ignore, per_image, kind):
    """The keys 1 - x s are one correctly rounded operation: the same on both sides, so the ranks are the reference's in f32."""
    loss, _ = check_case("binary", shape, ignore, per_image, kind)
    logits, y = H.binary_case(shape, ignore, kind)
    assert (y == 1).any() == (kind == "mixed")
    crit = gnn.LovaszLoss("binary", per_image=per_image, ignore_index=ignore)
    # a [B, H, W]-shaped target with equal numel is the same; any value other than 1 and ignore_index counts as 0
    assert torch.equal(crit(logits.to(DEV), y[:, 0].to(DEV)), loss.detach())
    other = y.clone()
    other[y == 0] = 7
    assert torch.equal(crit(logits.to(DEV), other.to(DEV)), loss.detach())
    with pytest.raises(ValueError, match="do not match"):
        crit(logits.to(DEV), y[:, :, :1].to(DEV))


def test_binary_ranks_are_exact():
    """coef = g_rank(i) in pixel order: from the CPU's stable sort of the same f32 keys it is the reference's to the last f32 bit of
    an f64 division."""
    logits, y = H.binary_case((2, 1, 37, 41), 255, "mixed")
    _, coef, norm = ops.lovasz_binary_fwd(logits.to(DEV), y.to(DEV), ops.LovaszOptions(False, 255))
    valid, z = (y != 255).reshape(-1), (y == 1).reshape(-1)
    e = torch.relu(1.0 - logits.reshape(-1) * (2.0 * z.float() - 1.0)) * valid
    perm = torch.sort(e, descending=True, stable=True)[1]
    want = torch.empty(e.numel(), dtype=torch.float64)
    want[perm] = H.jaccard_coef((z & valid)[perm], torch.float64)
    assert torch.equal(coef.cpu(), want.float()) and norm.cpu().tolist() == [1.0]


# ------------------------------------------------------------------------------------------------ 5. edge semantics
@pytest.mark.parametrize("per_image", [False, True])
def test_every_pixel_ignored(per_image):
    y = torch.full((2, 32, 32), 255, dtype=torch.int64, device=DEV)
    ld = (rnd(2, 5, 32, 32) * 2).to(DEV).requires_grad_(True)
    loss = gnn.LovaszLoss("multiclass", per_image=per_image, ignore_index=255)(ld, y)
    (UP * loss).backward()
    assert loss.item() == 0.0 and (ld.grad == 0).all()
    lb = (rnd(2, 1, 32, 32) * 2).to(DEV).requires_grad_(True)
    loss = gnn.LovaszLoss("binary", per_image=per_image, ignore_index=255)(lb, y)
    (UP * loss).backward()
    assert loss.item() == 0.0 and (lb.grad == 0).all()


def test_absent_class_is_skipped_and_out_of_range_target_matches_no_class():
    B, K, Hh, W = 2, 5, 24, 40
    logits = rnd(B, K, Hh, W, seed=K) * 2
    y = make_target((B, Hh, W), K - 1)                    # class 4 is absent
    g = torch.Generator().manual_seed(9)
    pick = torch.rand(y.shape, generator=g)
    y[pick < 0.05] = K                                    # one past the last class
    y[(pick >= 0.05) & (pick < 0.10)] = -3
    y[(pick >= 0.10) & (pick < 0.12)] = 2**33 + 1         # class 1 as a 32-bit value
    x = logits.double().requires_grad_(True)
    ref = H.lovasz_ref(x, y)                              # compares the target too: four present classes, no match for the rest
    (UP * ref).backward()
    ld = logits.to(DEV).requires_grad_(True)
    loss, coef, norm = ops.lovasz_fwd(ld.detach(), y.to(DEV))
    assert norm.cpu().tolist() == [0.25, 0.25, 0.25, 0.25, 0.0]
    out = gnn.LovaszLoss("multiclass")(ld, y.to(DEV))
    (UP * out).backward()
    assert torch.equal(out.detach(), loss)
    assert abs(loss.item() - ref.item()) <= LOSS_TOL["multiclass"]
    assert (ld.grad.cpu().double() - x.grad).abs().max().item() <= GRAD_TOL["multiclass"] * x.grad.abs().max().item()


@pytest.mark.parametrize("K", [5, 19])
def test_saturated_logits_stay_finite(K):
    """Every logit is +80 or -80: probabilities of exactly 0 and 1, most keys exactly 0 or 1 (ranks by index)."""
    B, Hh, W = 2, 21, 23
    g = torch.Generator().manual_seed(5)
    logits = (torch.randint(0, 2, (B, K, Hh, W), generator=g).float() * 2 - 1) * 80.0
    y = make_target((B, Hh, W), K, 255)
    x = logits.double().requires_grad_(True)
    ref = H.lovasz_ref(x, y, ignore_index=255)
    (UP * ref).backward()
    ld = logits.to(DEV).requires_grad_(True)
    loss = gnn.LovaszLoss("multiclass", ignore_index=255)(ld, y.to(DEV))
    (UP * loss).backward()
    assert torch.isfinite(loss).item() and torch.isfinite(ld.grad).all().item()
    assert abs(loss.item() - ref.item()) <= LOSS_TOL["multiclass"]
    assert (ld.grad.cpu().double() - x.grad).abs().max().item() <= GRAD_TOL["multiclass"] * x.grad.abs().max().item()
    lb = logits[:, :1].contiguous().to(DEV).requires_grad_(True)
    loss = gnn.LovaszLoss("binary", ignore_index=255)(lb, y.to(DEV))
    loss.backward()
    assert torch.isfinite(loss).item() and torch.isfinite(lb.grad).all().item()


# ------------------------------------------------------------------------------------------------ 6. determinism and plumbing
def test_two_calls_give_the_same_bits():
    up = torch.tensor(UP, device=DEV)
    for per_image in (False, True):
        opt = ops.LovaszOptions(per_image, 255)
        logits, y = (rnd(2, 5, 129, 64) * 2).to(DEV), make_target((2, 129, 64), 5, 255).to(DEV)
        runs = []
        for _ in range(2):
            loss, coef, norm = ops.lovasz_fwd(logits, y, opt)
            runs.append((loss, coef, norm, ops.lovasz_bwd(logits, y, coef, norm, up, 1.0, opt)))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), per_image
        lb, yb = logits[:, :1].contiguous(), make_target((2, 1, 129, 64), 2, 255).to(DEV)
        runs = []
        for _ in range(2):
            loss, coef, norm = ops.lovasz_binary_fwd(lb, yb, opt)
            runs.append((loss, coef, norm, ops.lovasz_binary_bwd(lb, yb, coef, norm, up, 1.0, opt)))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), per_image


def test_backward_accumulates_into_an_existing_gradient():
    up = torch.tensor(UP, device=DEV)
    logits, y = (rnd(2, 5, 20, 20) * 2).to(DEV), make_target((2, 20, 20), 5).to(DEV)
    _, coef, norm = ops.lovasz_fwd(logits, y)
    g = ops.lovasz_bwd(logits, y, coef, norm, up, 0.5)
    acc = torch.ones_like(logits)
    ops.lovasz_bwd(logits, y, coef, norm, up, 0.5, out=acc, accumulate=True)
    assert g.abs().max().item() > 0 and torch.equal(acc, 1.0 + g)
    lb, yb = logits[:, :1].contiguous(), make_target((2, 1, 20, 20), 2).to(DEV)
    _, coef, norm = ops.lovasz_binary_fwd(lb, yb)
    g = ops.lovasz_binary_bwd(lb, yb, coef, norm, up, 0.5)
    acc = torch.ones_like(lb)
    ops.lovasz_binary_bwd(lb, yb, coef, norm, up, 0.5, out=acc, accumulate=True)
    assert g.abs().max().item() > 0 and torch.equal(acc, 1.0 + g)


def test_c_entry_points_return_error_codes():
    lib = gdlhip._lib.load()
    x, y = torch.zeros(1, 3, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV)
    buf = torch.zeros(4096, device=DEV)
    p, none, opt = (lambda t: t.data_ptr()), None, (0, 0, 0)
    assert lib.gdl_sort_desc_workspace(0, 16) == 0 and lib.gdl_sort_desc_workspace(1, 0) == 0 and lib.gdl_sort_desc_workspace(1, 16) > 0
    assert lib.gdl_lovasz_workspace(3, 0, 3) == 0 and lib.gdl_lovasz_workspace(3, 16, 0) == 0 and lib.gdl_lovasz_workspace(4, 16, 3) == 0
    need = lib.gdl_lovasz_workspace(3, 16, 3)
    assert 0 < need <= buf.numel() * 4
    bad = [
        lib.gdl_sort_desc_f32(none, 1, 16, p(buf), p(buf), p(buf), 16384, none),                        # null keys
        lib.gdl_sort_desc_f32(p(buf), 1, 0, p(buf), p(buf), p(buf), 16384, none),                       # n = 0
        lib.gdl_sort_desc_f32(p(buf), 0, 16, p(buf), p(buf), p(buf), 16384, none),                      # S = 0
        lib.gdl_sort_desc_f32(p(x), 1, 16, p(buf), p(buf[1024:]), p(buf[2048:]), 8, none),              # workspace too small
        lib.gdl_lovasz_fwd(none, p(y), 1, 3, 16, *opt, p(buf), p(buf), p(buf), p(buf), 16384, none),    # null logits
        lib.gdl_lovasz_fwd(p(x), p(y), 1, 0, 16, *opt, p(buf), p(buf), p(buf), p(buf), 16384, none),    # K < 1
        lib.gdl_lovasz_fwd(p(x), p(y), 1, 3, 0, *opt, p(buf), p(buf), p(buf), p(buf), 16384, none),     # HW = 0
        lib.gdl_lovasz_fwd(p(x), p(y), 1, 3, 16, *opt, p(buf), p(buf), p(buf), p(buf), need - 1, none),  # workspace too small
        lib.gdl_lovasz_bwd(p(x), p(y), 1, 3, 16, *opt, none, p(buf), none, 1.0, p(buf), 0, none),       # null coef
        lib.gdl_lovasz_bwd(p(x), p(y), 0, 3, 16, *opt, p(buf), p(buf), none, 1.0, p(buf), 0, none),     # B = 0
        lib.gdl_lovasz_binary_fwd(p(x), p(y), 1, 0, *opt, p(buf), p(buf), p(buf), p(buf), 16384, none),  # no logits
        lib.gdl_lovasz_binary_fwd(p(x), none, 1, 16, *opt, p(buf), p(buf), p(buf), p(buf), 16384, none),
        lib.gdl_lovasz_binary_bwd(p(x), p(y), 1, 16, *opt, p(buf), p(buf), none, 1.0, none, 0, none),   # null dlogits
    ]
    assert all(rc != 0 for rc in bad), bad      # GDL_OK = 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.sort_desc_f32(torch.zeros(1, 0, device=DEV))
    with pytest.raises(ValueError, match="target"):
        ops.lovasz_fwd(x, y[:, :2].contiguous())
    with pytest.raises(ValueError, match="coef"):
        ops.lovasz_bwd(x, y, buf[:7], buf[:3], None)


def test_checked_view_raises_where_the_raw_view_returns_the_status():
    """The null-logits call of the test above through both views of the binding: ``_lib.load()`` returns GDL_ERR_INVALID,
    ``_lib.checked()`` (what gdlhip.ops launches through) raises ValueError, the symbol first, then gdl_last_error()'s message.  The
    argument check returns before any launch."""
    raw, chk = gdlhip._lib.load(), gdlhip._lib.checked()
    y, buf = torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV), torch.zeros(4096, device=DEV)
    args = (None, y.data_ptr(), 1, 3, 16, 0, 0, 0, *[buf.data_ptr()] * 4, 16384, None)
    assert raw.gdl_lovasz_fwd(*args) == -1
    message = raw.gdl_last_error().decode()
    assert "null pointer" in message
    with pytest.raises(ValueError) as e:
        chk.gdl_lovasz_fwd(*args)
    assert str(e.value) == "gdl_lovasz_fwd: " + message and not isinstance(e.value, gdlhip.GdlHipError)
    assert chk.gdl_lovasz_workspace(3, 16, 3) == raw.gdl_lovasz_workspace(3, 16, 3) > 0      # a query: its value, unchecked


# ------------------------------------------------------------------------------------------------ 7. captured step
def test_graphed_train_step_reproduces_the_eager_losses_bit_for_bit():
    """GraphedTrainStep (hipGraph capture of forward + LovaszLoss + backward + Adam) on the toy task: one capture and three replays
    against the same steps run eagerly, bit for bit.  In a process of its own (tests/_loss_graph_worker.py, scenario "lovasz")."""
    worker = Path(__file__).with_name("_loss_graph_worker.py")
    run = subprocess.run([sys.executable, str(worker), "lovasz"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    print(res)
    assert len(res["eager"]) == 3 and res["eager"] == res["graphed"], res
