"""The input families and the float64 expectations of tests/test_hip_attention_exact.py, tested where there is no GPU: against
a naive float64 softmax attention and its autograd gradient, for representability in bf16, against a transcription of the
split-query rule, and for their sensitivity to one missing (or one invented) key."""

import math

import pytest
import torch

import test_hip_attention_exact as ex

HOST_SHAPES = [(1, 1, 1, 1), (1, 193, 2, 3), (31, 2, 2, 4), (33, 32, 2, 4), (63, 33, 2, 3), (64, 64, 1, 1), (65, 65, 2, 4),
               (64, 193, 2, 3), (129, 129, 2, 3), (257, 63, 2, 4), (257, 191, 1, 8), (257, 193, 2, 4)]


def naive(q, k, v, do=None):
    """softmax(q k^T / 8) v per batch and head in float64, P and LSE; with `do` the autograd gradients too."""
    q, k, v = (t.clone().requires_grad_(do is not None) for t in (q, k, v))
    s = torch.einsum("bihd,bjhd->bhij", q, k) * ex.SCALE
    P = s.softmax(-1)
    o = torch.einsum("bhij,bjhd->bihd", P, v)
    if do is None:
        return P, o, s.logsumexp(-1)
    o.backward(do)
    return P.detach(), o.detach(), s.logsumexp(-1).detach(), q.grad, k.grad, v.grad


def families(Nq, Nkv, B, H):
    yield "uniform", ex.uniform_inputs(B, H, Nq, Nkv)
    yield "routing", ex.routing_inputs(B, H, Nq, Nkv)
    yield "selection", ex.selection_inputs(B, H, Nq, Nkv)
    yield "dominant-last", ex.selection_inputs(B, H, Nq, Nkv, dominant=Nkv - 1)
    yield "dominant-first", ex.selection_inputs(B, H, Nq, Nkv, dominant=0)


def test_codes_are_orthogonal_and_start_with_plus_one():
    h = ex.hadamard()
    assert torch.equal(h @ h.T, 64.0 * torch.eye(64, dtype=torch.float64)) and bool((h.abs() == 1).all()) and bool((h[:, 0] == 1).all())
    rows = ex.coded(2, 130, 3)
    s = ex.scores(rows, rows)
    i = torch.arange(130)
    match = (i.view(-1, 1) % 64) == (i.view(1, -1) % 64)
    assert bool((s[:, :, match] == 32.0).all()) and bool((s[:, :, ~match] == 0.0).all())
    assert not torch.equal(rows[0, :, 0], rows[0, :, 1]) and not torch.equal(rows[0, :, 0], rows[1, :, 0])


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=[str(s) for s in HOST_SHAPES])
def test_forward_ideal_is_the_softmax_up_to_the_tail(shape):
    """P is 0 or 1/c up to the Nkv e^-32 weight of the non-matching keys; O and LSE follow; operands and the values claimed
    exact are bf16 numbers."""
    Nq, Nkv, B, H = shape
    for name, (q, k, v) in families(Nq, Nkv, B, H):
        r = ex.ideal(q, k, v)
        P, o, lse = naive(q, k, v)
        leak = Nkv * ex.EPS
        assert bool(((r.P == 0) | (r.P == 1.0 / r.c)).all()) and bool((r.P.sum(-1) - 1).abs().max() < 1e-15), name
        assert (P - r.P).abs().max().item() <= leak, name
        assert (o - r.o).abs().max().item() <= r.tail_o + 1e-13 * v.abs().max().item(), name   # (+ float64 rounding of the naive sums)
        assert (lse - r.lse).abs().max().item() <= leak + 1e-14, name
        assert (r.tail_o == 0.0) == name.startswith(("uniform", "routing")) or Nkv == 1, name
        for t in (q, k, v):
            assert torch.equal(ex.rb(t), t), name
        claimed = r.o[r.pow2 & ex.representable(r.o)]
        assert torch.equal(ex.rb(claimed), claimed)
        if name.startswith("dominant"):
            pos = Nkv - 1 if name.endswith("last") else 0
            assert torch.equal(r.o, v[:, pos:pos + 1].expand_as(r.o)) and bool((r.lse == 64.0).all())
        if name == "routing":
            ident = (1 + torch.arange(B * H)).double().view(B, 1, H, 1).expand_as(r.o)
            assert torch.equal(r.o, ident)
        if name == "selection" and Nkv <= 128:
            assert set(r.c.unique().tolist()) <= {1.0, 2.0, float(Nkv)}
            assert bool(ex.representable(r.o[r.pow2]).all()), "means of two even integers are integers"


def test_uniform_family_counts_keys():
    q, k, v = ex.uniform_inputs(2, 3, 5, 193)
    r = ex.ideal(q, k, v)
    w = ex.head_weight(2, 3)
    j = torch.arange(193)
    count = torch.zeros(64, dtype=torch.float64).index_add_(0, j % 64, (1 + (j // 64) % 3).double())
    assert torch.allclose(r.o, (w * count / 193).expand_as(r.o), rtol=1e-15, atol=0)
    assert bool((r.lse == math.log(193)).all())
    q, k, v = ex.uniform_inputs(1, 1, 3, 31)
    assert bool((ex.ideal(q, k, v).o[..., 31:] == 0).all()), "channels without a key are exactly 0"


@pytest.mark.parametrize("case", [c for c in ex.BWD_CASES if c[0] <= 1025], ids=[i for c, i in zip(ex.BWD_CASES, ex.BWD_IDS) if c[0] <= 1025])
def test_backward_ideal_is_the_autograd_gradient_up_to_the_tail(case):
    """ideal() asserts that P, dS and O round to bf16 exactly and that the sums are exact in f32; here its gradients are
    held against the float64 autograd gradient of the naive attention within tail_backward (the weight of non-matching keys)."""
    Nq, Nkv, B, H = case[:4]
    q, k, v, do, r = ex.backward_problem(Nq, Nkv, B, H)
    P, o, lse, dq, dk, dv = naive(q, k, v, do)
    assert (P - r.P).abs().max().item() <= Nkv * ex.EPS
    assert set(r.c.unique().tolist()) <= {1.0, 2.0}
    tail = ex.tail_backward(Nq, Nkv)
    assert tail < 2.0 ** -24, "the tail allowance stays nine orders below the smallest non-zero ideal element (>= 2^-8)"
    for name, a, b in (("dq", dq, r.dq), ("dk", dk, r.dk), ("dv", dv, r.dv)):
        assert (a - b).abs().max().item() <= tail / 4, (name, (a - b).abs().max().item(), tail)
        nz = b[b != 0].abs()
        assert nz.numel() == 0 or nz.min().item() >= 2.0 ** -8, name
    for name, allow, want in (("o", r.a_o, r.o), ("dq", r.a_dq, r.dq), ("dk", r.a_dk, r.dk), ("dv", r.a_dv, r.dv)):
        nz = want[want != 0].abs()
        if nz.numel():
            assert allow.max().item() < 2.0 ** -9 * nz.min().item(), (name, allow.max().item(), nz.min().item())
    one_match = (r.c == 1).expand_as(r.dS)
    assert bool((r.dS[one_match] == 0).all()), "dS is exactly 0 on one-match rows"
    if Nkv > 64:
        assert bool((r.dS != 0).any()), "two-match rows must give the backward something to compute"
    for t in (do, r.o, r.P, r.dS):
        assert torch.equal(ex.rb(t), t)


@pytest.mark.parametrize("case", [c for c in ex.BWD_CASES if c[0] > 1025], ids=[i for c, i in zip(ex.BWD_CASES, ex.BWD_IDS) if c[0] > 1025])
def test_large_backward_cases_build(case):
    Nq, Nkv, B, H = case[:4]
    r = ex.backward_problem(Nq, Nkv, B, H)[4]
    assert bool((r.dk != 0).any()) and bool((r.dv != 0).any()) and ex.tail_backward(Nq, Nkv) < 2.0 ** -24
    for name, allow, want in (("o", r.a_o, r.o), ("dq", r.a_dq, r.dq), ("dk", r.a_dk, r.dk), ("dv", r.a_dv, r.dv)):
        nz = want[want != 0].abs()
        # (dK of these cases sums 25 / 65 query tiles, each with its inherited share: 2^-5 instead of 2^-9)
        assert nz.numel() == 0 or allow.max().item() < 2.0 ** -5 * nz.min().item(), (name, allow.max().item(), nz.min().item())


def test_split_counts_are_those_of_the_rule():
    """The table's split counts equal the transcription of dkv_qsplit and the library's own workspace query (a host
    function); the classes the issue asks for are all present."""
    from gdlhip import _lib
    lib = _lib.load()
    seen = set()
    for Nq, Nkv, B, H, want, empty, last in ex.BWD_CASES:
        assert ex.dkv_qsplit_py(B, H, Nq, Nkv) == want
        nbytes = lib.gdl_flash_attn_bwd_workspace(B, H, Nq, Nkv)
        assert nbytes == (want * B * H * Nkv * 512 if want > 1 else 0)
        e, l, per = ex.last_parts(Nq, want)
        assert (e, (l, per)) == (empty, last)
        assert Nkv <= 128 and (Nkv >= 64 or Nq <= Nkv)
        seen.add("1" if want == 1 else "2" if want == 2 else "3-15" if want < 16 else "16")
        if e:
            seen.add(f"empty{e}")
        if l < per:
            seen.add("short")
    assert seen >= {"1", "2", "3-15", "16", "empty1", "empty3", "short"}
    assert ex.dkv_qsplit_py(1, 1, 1600, 128) == 6 and ex.last_parts(1600, 6) == (1, 5, 5)
    assert ex.dkv_qsplit_py(1, 32, 4160, 128) == 16 and ex.last_parts(4160, 16) == (3, 5, 5)
    assert ex.dkv_qsplit_py(86, 1, 1600, 128) == 6 and ex.dkv_qsplit_py(103, 1, 1600, 128) == 5


def test_shape_lists():
    ex.test_shape_list_covers_the_edges()
    for Nq, Nkv, B, H in ex.POISON:
        ex.backward_problem(Nq, Nkv, B, H)        # (ideal() asserts that the shape suits the backward model)
    assert {c[0] for c in ex.BWD_CASES} >= {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 1600, 4160}
    assert max(s[2] * s[3] for s in ex.SHAPES) <= 16 and max(c[2] * c[3] for c in ex.BWD_CASES) <= 16


def test_compare_is_per_element():
    want = torch.tensor([3.0, 1.0 / 3, 0.0, 100.0, 0.375], dtype=torch.float64)
    good = ex.rb(want)
    ex.compare(good, want, True, 0.0, "good", quiet=True)
    step = ex.ulp_bf16(want)
    assert step.tolist() == [2.0 ** -6, 2.0 ** -9, 2.0 ** -8, 2.0 ** -1, 2.0 ** -9]
    for i, delta in ((0, step[0].item()), (1, 2.1 * step[1].item()), (2, 1e-30), (4, step[4].item())):
        bad = good.clone()
        bad[i] += delta
        with pytest.raises(AssertionError):
            ex.compare(bad, want, True, 0.0, "bad", quiet=True)
    ok = good.clone()
    ok[2] = 1e-12                  # an ideal 0 next to keys 32 below the maximum: the e^-32 tail, and no more than it
    ex.compare(ok, want, True, 1e-11, "tail", quiet=True)
    with pytest.raises(AssertionError):
        ok[0] += 1e-3              # far below any tensor-wide tolerance, and still refused
        ex.compare(ok, want, True, 1e-11, "tail", quiet=True)


def test_one_missing_or_invented_key_is_seen():
    """Largest Nkv in use (193): deleting any one key from the reference moves some output element of the uniform family by
    more than two bf16 ulps (the one-ulp allowance cannot cover it) and LSE by more than 0.25 / Nkv; so does one phantom
    key of score 0 (what a key mask `key <= N` lets in: the staged row behind the last key is zeros).  compare() and
    compare_lse() refuse both."""
    B, H, Nq, Nkv = 1, 2, 3, 193
    q, k, v = ex.uniform_inputs(B, H, Nq, Nkv)
    r = ex.ideal(q, k, v)
    ex.compare(ex.rb(r.o), r.o, r.pow2, 0.0, "ideal", quiet=True)
    mutants = [(torch.cat([k[:, :j], k[:, j + 1:]], 1), torch.cat([v[:, :j], v[:, j + 1:]], 1)) for j in (0, 63, 64, 100, 191, 192)]
    for km, vm in mutants:
        _, o, lse = naive(q, km, vm)
        moved = ((o - r.o).abs() / ex.ulp_bf16(r.o))[r.o != 0].max().item()
        assert moved > 2.0, moved
        assert (lse - r.lse).abs().min().item() > 0.25 / Nkv
        with pytest.raises(AssertionError):
            ex.compare(ex.rb(o), r.o, r.pow2, 0.0, "mutant", quiet=True)
        with pytest.raises(AssertionError):
            ex.compare_lse(lse, r, "mutant")
    # one phantom key of score 0 and V = 0 only turns the divisor Nkv into Nkv + 1: at 193 keys that is 1.3 bf16 ulps of O, which
    # the LSE bound catches (ln(194 / 193) is four times 0.25 / Nkv); up to 65 keys O itself moves by more than two ulps
    for n in (193, 65, 63, 33, 2, 1):
        q, k, v = ex.uniform_inputs(B, H, Nq, n)
        r = ex.ideal(q, k, v)
        _, o, lse = naive(q, torch.cat([k, torch.zeros_like(k[:, :1])], 1), torch.cat([v, torch.zeros_like(v[:, :1])], 1))
        with pytest.raises(AssertionError):
            ex.compare_lse(lse, r, "phantom key")
        if n <= 65:
            assert ((o - r.o).abs() / ex.ulp_bf16(r.o))[r.o != 0].min().item() > 2.0
            with pytest.raises(AssertionError):
                ex.compare(ex.rb(o), r.o, r.pow2, 0.0, "phantom key", quiet=True)
    # the selection family sees the phantom key too wherever a query has no matching key (uniform rows), and a lost key always
    q, k, v = ex.selection_inputs(1, 1, 65, 193)
    r = ex.ideal(q, k, v)
    _, o, _ = naive(q, k[:, :-1], v[:, :-1])
    with pytest.raises(AssertionError):
        ex.compare(ex.rb(o), r.o, r.pow2, r.tail_o, "mutant", quiet=True)


def test_phantom_query_of_the_dkv_kernel_is_inert():
    """A query mask `<= Nq` in flash_bwd_dkv_kernel admits the row behind the last query.  That row is staged as zeros (Q = 0,
    dO = 0) with LSE = dvec = 0 in the LDS: P = exp(0 - 0) = 1, but dV += P dO = 0 and dS = P (0 - 0) / 8 = 0 -- the mutant
    computes the same gradients, no test can tell it apart."""
    Nq, Nkv, B, H = 65, 65, 1, 1
    q, k, v, do, r = ex.backward_problem(Nq, Nkv, B, H)
    P_row = torch.ones(B, H, 1, Nkv, dtype=torch.float64)
    do_row, q_row = torch.zeros(B, 1, H, 64, dtype=torch.float64), torch.zeros(B, 1, H, 64, dtype=torch.float64)
    dS_row = P_row * (torch.einsum("bihd,bjhd->bhij", do_row, v) - 0.0) * ex.SCALE
    assert torch.equal(r.dv + torch.einsum("bhij,bihd->bjhd", P_row, do_row), r.dv)
    assert torch.equal(r.dk + torch.einsum("bhij,bihd->bjhd", dS_row, q_row), r.dk)
