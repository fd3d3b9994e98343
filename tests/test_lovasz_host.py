"""gdlhip.nn.LovaszLoss, the parts that need no GPU: the reference the GPU tests hold the kernels against, the constructor contract,
the config alias and ``reads_lowres``; and the data of the GPU cases (tests/test_hip_lovasz.py), so that their f32-vs-f64 deviation
can be measured on the CPU (``python tests/test_lovasz_host.py`` prints it).

Reference: ``lovasz_ref``, the definition in ``gdlhip.nn.LovaszLoss``'s docstring restated with torch in the dtype of the logits:
softmax (or the hinge), ``torch.sort(descending=True, stable=True)``, the Jaccard coefficients from exact integer counts in the
cancellation-free form, ignored pixels REMOVED before the sort (smp's compaction; the kernels keep them as zero keys instead).
The gradient is torch autograd's with the coefficients detached.  smp itself is not available, so parity with it is unpinned; what
is pinned here is that the restatement equals an independent O(n^2) evaluation of the Lovasz extension of the Jaccard loss."""

import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

_PKG = Path(__file__).resolve().parents[1] / "geo-deep-learning_amd"      # (conftest.py does this under pytest; this is for the script use)
if str(_PKG) not in sys.path:
    sys.path.insert(0, str(_PKG))
gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402


# ------------------------------------------------------------------------------------------------ the reference
def jaccard_coef(z_sorted, dtype):
    """g_r for the label bits in sorted order: 1 / U (z = 1), I / ((U - 1) U) (z = 0); G = 0: g_0 = 1, the rest 0.  Counts are exact
    int64; only the last division is in ``dtype``."""
    z = z_sorted.long()
    n, G = z.numel(), int(z.sum())
    if G == 0:
        g = torch.zeros(n, dtype=dtype)
        g[0] = 1.0
        return g
    P = z.cumsum(0)
    N = torch.arange(1, n + 1) - P
    inter, U = G - P, G + N
    pos = 1.0 / U.to(dtype)
    neg = inter.to(dtype) / ((U - 1) * U).clamp(min=1).to(dtype)
    return torch.where(z == 1, pos, neg)


def _segment_loss(e, z):
    es, perm = torch.sort(e, descending=True, stable=True)
    return (es * jaccard_coef(z[perm], e.dtype)).sum()


def _multiclass_flat(p, y, ignore_index):
    """p [n, K], y [n]: the mean over the present classes, ignored pixels removed first."""
    if ignore_index is not None:
        keep = y != ignore_index
        p, y = p[keep], y[keep]
    losses = [_segment_loss(((y == c).to(p.dtype) - p[:, c]).abs(), y == c) for c in range(p.shape[1]) if (y == c).any()]
    return torch.stack(losses).mean() if losses else p.sum() * 0.0


def _binary_flat(x, y, ignore_index):
    if ignore_index is not None:
        keep = y != ignore_index
        x, y = x[keep], y[keep]
    if y.numel() == 0:
        return x.sum() * 0.0
    z = y == 1
    return _segment_loss(torch.relu(1.0 - x * (2.0 * z.to(x.dtype) - 1.0)), z)


def lovasz_ref(logits, target, mode="multiclass", per_image=False, ignore_index=None):
    """The loss in the dtype of ``logits`` (a 0-dim tensor that autograd can walk back to ``logits``)."""
    B = logits.shape[0]
    if mode == "binary":
        x, y = logits.reshape(B, -1), target.reshape(B, -1)
        if per_image:
            return torch.stack([_binary_flat(x[b], y[b], ignore_index) for b in range(B)]).mean()
        return _binary_flat(x.reshape(-1), y.reshape(-1), ignore_index)
    K = logits.shape[1]
    y = (target[:, 0] if target.dim() == logits.dim() else target).reshape(B, -1)
    p = torch.softmax(logits, dim=1).reshape(B, K, -1).permute(0, 2, 1)      # [B, HW, K]
    if per_image:
        return torch.stack([_multiclass_flat(p[b], y[b], ignore_index) for b in range(B)]).mean()
    return _multiclass_flat(p.reshape(-1, K), y.reshape(-1), ignore_index)


def lovasz_extension_bruteforce(e, z):
    """sum_r e_(r) (J(M_r) - J(M_{r-1})) with M_r = the r + 1 largest errors and J(M) = 1 - |gt minus M| / |gt union M| evaluated
    from the sets themselves at every r: O(n^2), NumPy f64, no cumulative sums."""
    e, z = np.asarray(e, dtype=np.float64), np.asarray(z, dtype=bool)
    order = sorted(range(len(e)), key=lambda i: (-e[i], i))
    gt = set(np.flatnonzero(z).tolist())

    def jaccard_loss(mis):
        if not gt and not mis:
            return 0.0
        return 1.0 - len(gt - mis) / len(gt | mis)
    total, prev = 0.0, 0.0
    for r in range(len(order)):
        cur = jaccard_loss(set(order[:r + 1]))
        total += e[order[r]] * (cur - prev)
        prev = cur
    return total


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)))


def make_target(shape, k, ignore=None, frac=0.2, seed=1):
    """Random classes; with ``ignore``: a fifth of the pixels and the first two rows of every image ignored."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, k, shape, generator=g)
    if ignore is not None:
        t[torch.rand(shape, generator=g) < frac] = ignore
        t[..., :2, :] = ignore
    return t


SORT_TILE = 2048            # keys per workgroup of a radix pass (csrc/loss_lovasz.hip)
SCAN_TABLE_TILE = 2048      # entries of the (digit, workgroup) table one scan workgroup takes: more than 8 tiles -> three kernels
MULTI_SCAN_N = 8 * SORT_TILE + 1

_ALL = [(ig, pi, std) for ig in (None, 255, -1) for pi in (False, True) for std in (2.0, 6.0)]
# (shape [B, K, H, W], ignore_index, per_image, logit std)
MULTICLASS_CASES = (
    [((2, 5, 24, 40), *o) for o in _ALL] + [((1, 3, 16, 16), *o) for o in _ALL]
    + [((3, 16, 40, 24), *o) for o in ((None, False, 2.0), (255, True, 6.0), (-1, False, 6.0), (255, False, 2.0))]
    + [((2, K, 24, 40), *o) for K in (2, 16, 19) for o in ((255, False, 2.0), (None, True, 6.0))]
    # B H W = 16512 > 8 tiles: the table scan takes its multi-workgroup path (per_image: 8256 per segment, the single one)
    + [((2, 3, 129, 64), *o) for o in ((None, False, 2.0), (255, False, 6.0), (-1, True, 2.0), (255, True, 6.0))])
assert 2 * 129 * 64 >= MULTI_SCAN_N
# (shape, ignore_index, per_image, target kind)
BINARY_CASES = [((2, 1, 37, 41), ig, pi, kind) for ig in (None, 255) for pi in (False, True) for kind in ("mixed", "background")] + \
    [((1, 1, 129, 128), 255, False, "mixed")]


def multiclass_case(shape, ignore, std):
    B, K, H, W = shape
    return rnd(*shape, seed=K) * std, make_target((B, H, W), K, ignore)


def binary_case(shape, ignore, kind):
    logits = rnd(*shape, seed=1) * 2.0
    y = make_target(shape, 2, ignore)
    if kind == "background":
        y[y == 1] = 0
    return logits, y


@functools.lru_cache(maxsize=None)
def reference(mode, shape, ignore, per_image, extra, dtype=torch.float64, upstream=1.0):
    """(loss, d(upstream * loss) / d logits) of a case by ``lovasz_ref`` in ``dtype``; computed once per case and shared: do not
    write into the result."""
    logits, y = multiclass_case(shape, ignore, extra) if mode == "multiclass" else binary_case(shape, ignore, extra)
    x = logits.to(dtype).requires_grad_(True)
    loss = lovasz_ref(x, y, mode, per_image, ignore)
    (upstream * loss).backward()
    return loss.detach(), x.grad


def f32_deviation(mode, shape, ignore, per_image, extra):
    """(|loss32 - loss64|, max|grad32 - grad64| / max|grad64|) of the restatement run in f32 against itself in f64."""
    l64, g64 = reference(mode, shape, ignore, per_image, extra)
    l32, g32 = reference(mode, shape, ignore, per_image, extra, torch.float32)
    return abs(l32.double().item() - l64.item()), ((g32.double() - g64).abs().max() / g64.abs().max().clamp(min=1e-300)).item()


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("n", [1, 2, 7, 33, 64])
@pytest.mark.parametrize("kind", ["random", "ties", "no_positive", "all_positive"])
def test_restatement_equals_the_bruteforce_lovasz_extension(n, kind):
    g = torch.Generator().manual_seed(n)
    e = torch.rand(n, generator=g, dtype=torch.float64)
    z = torch.rand(n, generator=g) < 0.4
    if kind == "ties":
        e = (e * 3).floor() / 3          # three distinct values: ranks come from the index order
    elif kind == "no_positive":
        z[:] = False
    elif kind == "all_positive":
        z[:] = True
    want = lovasz_extension_bruteforce(e.numpy(), z.numpy())
    assert abs(_segment_loss(e, z).item() - want) <= 1e-14
    # the coefficients are the increments of J, sum to J(everything) = 1 and are never negative
    coef = jaccard_coef(z[torch.sort(e, descending=True, stable=True)[1]], torch.float64)
    assert abs(coef.sum().item() - 1.0) <= 1e-14 and (coef >= 0).all()


def test_multiclass_and_binary_restatements_on_small_inputs():
    """lovasz_ref against the brute force per class / image, ignored pixels dropped by hand, absent classes skipped."""
    x, y = rnd(2, 4, 3, 5) * 2, make_target((2, 3, 5), 3, 255)      # class 3 is absent
    y[0, 2, 0] = 7                                                   # out of range, not ignored: matches no class
    p = torch.softmax(x.double(), 1)
    per_image = []
    for b in range(2):
        keep = (y[b] != 255).reshape(-1).numpy()
        ls = []
        for c in range(4):
            z = (y[b] == c).reshape(-1).numpy()[keep]
            if z.any():
                ls.append(lovasz_extension_bruteforce(np.abs(z - p[b, c].reshape(-1).numpy()[keep]), z))
        per_image.append(sum(ls) / len(ls))
    got = lovasz_ref(x.double(), y, "multiclass", True, 255)
    assert abs(got.item() - sum(per_image) / 2) <= 1e-14
    xb, yb = rnd(2, 1, 3, 5) * 2, make_target((2, 1, 3, 5), 2, 255)
    keep = (yb != 255).reshape(-1).numpy()
    z = (yb == 1).reshape(-1).numpy()[keep]
    e = np.maximum(0.0, 1.0 - xb.double().reshape(-1).numpy()[keep] * (2.0 * z - 1.0))
    assert abs(lovasz_ref(xb.double(), yb, "binary", False, 255).item() - lovasz_extension_bruteforce(e, z)) <= 1e-14
    # ignored pixels as ZERO KEYS with label bit 0 (what the kernels do) give the loss of the compaction
    full_z = (yb == 1).reshape(-1)
    full_e = torch.relu(1.0 - xb.double().reshape(-1) * (2.0 * full_z.double() - 1.0)) * (yb != 255).reshape(-1)
    assert abs(_segment_loss(full_e, full_z & (yb != 255).reshape(-1)).item() - lovasz_extension_bruteforce(e, z)) <= 1e-14
    # nothing valid: 0
    none = torch.full_like(y, 255)
    assert lovasz_ref(x.double(), none, "multiclass", False, 255).item() == 0.0
    assert lovasz_ref(xb.double(), torch.full_like(yb, 255), "binary", True, 255).item() == 0.0


# ------------------------------------------------------------------------------------------------ the class
def test_constructor_accepts_smp_arguments_and_rejects_the_rest():
    crit = gnn.LovaszLoss("multiclass")
    assert (crit.mode, crit.per_image, crit.ignore_index, crit.from_logits) == ("multiclass", False, None, True)
    assert crit.options == ops.LovaszOptions(False, None) and crit.options.c_args() == (0, 0, 0)
    crit = gnn.LovaszLoss("binary", per_image=True, ignore_index=255)
    assert crit.options == ops.LovaszOptions(True, 255) and crit.options.c_args() == (1, 1, 255)
    assert gnn.LovaszLoss("multiclass", ignore_index=-1).options.c_args() == (0, 1, -1)
    assert ops.LovaszOptions._fields == ("per_image", "ignore_index")
    for bad in (2.5, True, 2**63):
        with pytest.raises(ValueError, match="ignore_index"):
            gnn.LovaszLoss("multiclass", ignore_index=bad)
    with pytest.raises(ValueError, match="mode"):
        gnn.LovaszLoss("regression")


@pytest.mark.parametrize("kw", [dict(mode="multilabel"), dict(from_logits=False)])
def test_unimplemented_arguments_raise_and_name_what_is_implemented(kw):
    with pytest.raises(NotImplementedError, match="implements"):
        gnn.LovaszLoss(**{"mode": "multiclass", **kw})


def test_reads_lowres_is_false():
    assert not gnn.reads_lowres(gnn.LovaszLoss("multiclass"))
    assert not gnn.reads_lowres(gnn.LovaszLoss("binary"))


def test_config_alias_resolves_to_the_hip_loss():
    from geo_deep_learning import train as gdl_train
    crit = gdl_train.instantiate({"class_path": "segmentation_models_pytorch.losses.LovaszLoss",
                                  "init_args": {"mode": "multiclass", "per_image": True, "ignore_index": 255}})
    assert type(crit) is gnn.LovaszLoss and crit.options == ops.LovaszOptions(True, 255)


def test_ops_refuse_cpu_tensors():
    x, y = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    coef, up, norm = torch.zeros(48), torch.ones(()), torch.ones(3)
    for call in (lambda: ops.lovasz_fwd(x, y), lambda: ops.lovasz_bwd(x, y, coef, norm, up),
                 lambda: ops.lovasz_binary_fwd(x[:, :1], y), lambda: ops.lovasz_binary_bwd(x[:, :1], y, coef[:16], norm[:1], up),
                 lambda: ops.sort_desc_f32(torch.zeros(2, 8)),
                 lambda: gnn.LovaszLoss("multiclass")(x, y), lambda: gnn.LovaszLoss("binary")(x[:, :1], y)):
        with pytest.raises(ValueError):
            call()


if __name__ == "__main__":      # the figures behind LOSS_TOL / GRAD_TOL of tests/test_hip_lovasz.py
    worst = {}
    for mode, cases in (("multiclass", MULTICLASS_CASES), ("binary", BINARY_CASES)):
        for shape, ignore, per_image, extra in cases:
            dl, dg = f32_deviation(mode, shape, ignore, per_image, extra)
            print(f"{mode} {shape} ignore={ignore} per_image={per_image} {extra}: loss dev {dl:.3e}  grad dev {dg:.3e}")
            w = worst.setdefault(mode, [0.0, 0.0])
            w[0], w[1] = max(w[0], dl), max(w[1], dg)
    print({k: (f"{v[0]:.3e}", f"{v[1]:.3e}") for k, v in worst.items()})
