"""Structured-input tests of the flash attention kernels (csrc/attention_v2.hip) and of the v1 / unfused / materialised paths.

The operands are built so that the correct result is known per element: with Q = 0 every key has the weight 1/Nkv (a key that
is lost, counted twice or invented moves a count by one); with Q and K rows taken from 64 mutually orthogonal +-1 codes a
matching pair scores 32 and every other pair 0, so that a query averages exactly its c matching keys (c = 1, 2, ...), and one
"dominant" key (score 64 with every query) turns the whole softmax into the selection of one row.  ``ideal()`` computes that
answer in float64 from the structure (the set of maximal scores of each row), not from an exponential.

Every element is compared with ITS OWN expected value (``compare``), never with a tensor maximum:

* ``torch.equal`` where the arithmetic is exact: the expected value is a bf16 number and the row divides by a power of two;
* one bf16 ulp of the expected element where a rounding step is not exact (each use names its step);
* an expected 0 must be 0 -- except where keys of score max - 32 exist: their weight e^-32 = 1.3e-14 is an ordinary f32 / bf16
  number and the kernels rightly keep it.  An element whose ideal value is 0 then holds (a) that tail (``tail_forward`` /
  ``tail_backward``, about 1e-11: the ideal answer's own distance from the true softmax) and (b), where the 0 is a
  cancellation such as 1 - 1, what the f32 accumulator lost on the way: 1 + (-1e-14) leaves an MFMA as 1 - 2^-24, and the
  sum ends at -2^-24 instead of 0.  The allowance of such an element is computed for it alone in ``ideal()``: the tail,
  plus one f32 ulp of its own absolute sum per MFMA instruction behind it, plus what it inherits from zero elements
  upstream (O -> dvec -> dS).  It stays below 2^-9 of the smallest non-zero element of the same tensor (2^-5 for dK of the cases
  with 1600 and 4160 queries; the host companion asserts both), so nothing that the other elements would not catch can hide in it; a non-zero element absorbs all of this
  in its own rounding to bf16 and stays exact.
* LSE: |LSE - ideal| < 0.25 / Nkv, a quarter of what one missing key moves it by.

The launchers call the C ABI directly and own every buffer: LSE, dvec and the split-query workspace are NaN-filled before the
call, the split count of each backward case comes from ``gdl_flash_attn_bwd_workspace`` and is asserted.
"""

import contextlib
import functools
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import _lib, ops  # noqa: E402

DEV = "cuda"
HD = 64
SCALE = HD ** -0.5
GAP = 32.0                            # score of a matching pair above every other pair
EPS = math.exp(-GAP)                  # weight of one non-matching key relative to a matching one
NAN = float("nan")
BF16 = torch.bfloat16
F32_STEP = 2.0 ** -23                 # one f32 ulp of a partial sum in [1, 2): what one (truncating) MFMA accumulation may lose


# ------------------------------------------------------------------ number formats
def rb(x):
    """float64 -> nearest bf16 -> float64."""
    return x.to(BF16).double()


def representable(x):
    return rb(x) == x


def ulp_bf16(x):
    """Spacing of the bf16 numbers at |x| (8 significant bits): 2^(floor(log2 |x|) - 7)."""
    _, e = torch.frexp(x.abs())
    return torch.ldexp(torch.ones_like(x), e - 8)


# ------------------------------------------------------------------ input families: float64 [B, N, H, 64] on the CPU
@functools.lru_cache(maxsize=1)
def hadamard():
    """64 mutually orthogonal +-1 vectors (Sylvester); column 0 is all +1."""
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < HD:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def coded(B, N, H):
    """rows[b, n, h] = 2 * code((n + 5 (b H + h)) % 64): a pair (i, j) of one (b, h) matches iff i % 64 == j % 64; the shift
    gives every batch and head its own rows, so that K of another head matches nowhere in the same pattern."""
    n = torch.arange(N).view(1, N, 1)
    bh = torch.arange(B * H).view(B, 1, H)
    return 2.0 * hadamard()[(n + 5 * bh) % HD]


def head_weight(B, H):
    return (1 + torch.arange(B * H) % 3).double().view(B, 1, H, 1)


def ints(shape, seed, values):
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor(values, dtype=torch.float64)
    return vals[torch.randint(0, len(values), tuple(shape), generator=g)]


@functools.lru_cache(maxsize=None)
def uniform_inputs(B, H, Nq, Nkv):
    """Family 1.  Q = 0; V[b, j, h, d] = w(b, h) * (1 + (j // 64) % 3) at d == j % 64, else 0: channel d of the output
    counts (weighted by key tile) the keys j = d mod 64."""
    j = torch.arange(Nkv)
    rows = torch.zeros(Nkv, HD, dtype=torch.float64)
    rows[j, j % HD] = (1 + (j // HD) % 3).double()
    v = rows.view(1, Nkv, 1, HD) * head_weight(B, H)
    return torch.zeros(B, Nq, H, HD, dtype=torch.float64), coded(B, Nkv, H), v.contiguous()


@functools.lru_cache(maxsize=None)
def routing_inputs(B, H, Nq, Nkv):
    """Family 2.  Q = 0; V[b, :, h, :] = 1 + b H + h."""
    ident = (1 + torch.arange(B * H)).double().view(B, 1, H, 1)
    return (torch.zeros(B, Nq, H, HD, dtype=torch.float64), coded(B, Nkv, H),
            ident.expand(B, Nkv, H, HD).contiguous())


@functools.lru_cache(maxsize=None)
def selection_inputs(B, H, Nq, Nkv, dominant=None, signed=False):
    """Family 3.  Q[i] = 2 code(i % 64), K[j] = 2 code(j % 64).  V: positive even integers (means of two are integers, no
    ideal element is 0), or, for the backward, {-1, 0, 1}.  `dominant`: key position whose K row is 256 e_0 -- every code
    starts with +1, so it scores 2 * 256 / 8 = 64 with every query."""
    k = coded(B, Nkv, H).clone()
    if dominant is not None:
        k[:, dominant] = 0.0
        k[:, dominant, :, 0] = 256.0
    v = ints((B, Nkv, H, HD), 100 + Nkv, (-1.0, 0.0, 1.0) if signed else (2.0, 4.0, 6.0))
    return coded(B, Nq, H), k, v


@functools.lru_cache(maxsize=None)
def grad_output(B, H, Nq):
    return ints((B, Nq, H, HD), 200 + Nq, (-1.0, 0.0, 1.0))


# ------------------------------------------------------------------ the ideal answer (float64, from the structure)
def scores(q, k):
    return torch.einsum("bihd,bjhd->bhij", q, k) * SCALE


def ideal(q, k, v, do=None):
    """Ideal attention of structured inputs: each row weighs its M maximal-score keys 1/c each (c = their number) and every
    other key -- at least GAP below, asserted -- not at all.  With `do`: the ideal gradients as well, with the roundings
    the fused backward makes (P and dS to bf16 before the second GEMMs, O to bf16 by the forward) asserted EXACT, so the
    gradients are plain float64 sums of dyadic numbers that an f32 accumulator holds exactly in any order."""
    assert all(bool(representable(t).all()) for t in (q, k, v)), "operands must be bf16 numbers"
    B, Nq, H, _ = q.shape
    Nkv = k.shape[1]
    s = scores(q, k)
    mx = s.amax(-1, keepdim=True)
    M = s == mx
    assert bool((M | (s <= mx - GAP)).all()), "a score within GAP of its row's maximum"
    c = M.sum(-1, keepdim=True).double()
    r = SimpleNamespace(B=B, H=H, Nq=Nq, Nkv=Nkv, M=M, c=c, P=M.double() / c)
    r.o = torch.einsum("bhij,bjhd->bihd", M.double(), v) / c.squeeze(-1).permute(0, 2, 1).unsqueeze(-1)
    r.lse = (mx + c.log()).squeeze(-1)
    ci = c.squeeze(-1).long()
    r.pow2 = ((ci & (ci - 1)) == 0).permute(0, 2, 1).unsqueeze(-1).expand(B, Nq, H, HD)
    has_tail = bool((~M).any())
    r.tail_o = tail_forward(Nkv, v.abs().max().item()) if has_tail else 0.0
    steps_k, steps_q = -(-Nkv // 16), -(-Nq // 16)          # MFMA instructions (16 keys / queries each) behind one accumulator
    r.a_o = r.tail_o + F32_STEP * steps_k * torch.einsum("bhij,bjhd->bihd", r.P, v.abs())
    if do is None:
        return r
    assert max(t.abs().max().item() for t in (v, do)) <= 1 and max(t.abs().max().item() for t in (q, k)) <= 2
    r.tail_grad = tail_backward(Nq, Nkv) if has_tail else 0.0
    assert bool(representable(r.o).all()), "the forward's bf16 output must be exact"
    dP = torch.einsum("bihd,bjhd->bhij", do, v)
    r.dvec = torch.einsum("bihd,bihd->bhi", do, r.o)
    r.dS = r.P * (dP - r.dvec.unsqueeze(-1)) * SCALE
    assert bool(representable(r.P).all()) and bool(representable(r.dS).all()), "P / dS must round to bf16 exactly"
    # allowances of the elements whose ideal value is 0 (see the module docstring): the zero elements of O carry a_o, dvec
    # inherits it (an RNE sum moves by at most twice the noise it is fed), dS of a matching pair inherits dvec's
    d_dvec = 2.0 * torch.einsum("bihd,bihd->bhi", do.abs(), r.a_o * (r.o == 0))
    d_dS = r.P * d_dvec.unsqueeze(-1) * SCALE * (1 + 2.0 ** -7)
    r.a_dvec = r.tail_grad + d_dvec
    r.a_dq = r.tail_grad + torch.einsum("bhij,bjhd->bihd", d_dS + F32_STEP * steps_k * r.dS.abs(), k.abs())
    r.a_dk = r.tail_grad + torch.einsum("bhij,bihd->bjhd", d_dS + F32_STEP * steps_q * r.dS.abs(), q.abs())
    r.a_dv = r.tail_grad + F32_STEP * steps_q * torch.einsum("bhij,bihd->bjhd", r.P, do.abs())
    r.dq = torch.einsum("bhij,bjhd->bihd", r.dS, k)
    r.dk = torch.einsum("bhij,bihd->bjhd", r.dS, q)
    r.dv = torch.einsum("bhij,bihd->bjhd", r.P, do)
    # every term is a multiple of 2^-8 and the absolute sums stay below 2^15: exact in f32 whatever the order
    for g, a, b in ((r.dq, r.dS, k), (r.dk, r.dS, q), (r.dv, r.P, do)):
        assert bool((g * 256 == (g * 256).round()).all())
    assert torch.einsum("bhij,bihd->bjhd", r.dS.abs(), q.abs()).max().item() < 2 ** 15
    return r


def tail_forward(Nkv, vmax):
    """Bound of |O - ideal O|: at most Nkv keys of relative weight EPS each, once in the numerator (times max|V|) and
    once in the row sum that divides it."""
    return 2.0 * Nkv * EPS * vmax


def tail_backward(Nq, Nkv):
    """Bound of |gradient - ideal gradient| for |V|, |dO| <= 1 and |Q|, |K| <= 2 (asserted in ideal()).  A non-matching
    pair has P <= EPS and |dS| <= EPS (|dP| + |dvec|) / 8 <= 16 EPS: at most 32 EPS per term of dQ (Nkv terms) or dK (Nq
    terms), EPS per term of dV.  A matching pair inherits the forward's tail through dvec = sum_d dO O: |delta O| <= 2 Nkv
    EPS per channel, 128 Nkv EPS per row, 16 Nkv EPS in dS, 32 Nkv EPS per term of dQ (<= 2 terms) or dK (<= Nq / 64 + 1
    terms).  Sum: 32 EPS (Nq + Nkv (Nq / 64 + 2)); doubled for the bf16 rounding of each term and doubled again."""
    return 128.0 * EPS * (Nq + Nkv * (Nq / 64 + 2))


def compare(got, want, exact_mask, tail, what, quiet=False):
    """Per-element comparison of `got` (device tensor, any float dtype) with the float64 ideal `want`:
    want == 0 -> |got| <= tail (0 unless non-matching keys exist); want a bf16 number and exact_mask -> bit-equal;
    everything else -> |got - want| <= one bf16 ulp of want."""
    got = got.detach().double().cpu().reshape(want.shape)
    assert not bool(got.isnan().any()), f"{what}: {int(got.isnan().sum())} NaN"
    exact_mask = torch.as_tensor(exact_mask).expand(want.shape)
    tail = torch.as_tensor(tail, dtype=torch.float64).expand(want.shape)
    zero = want == 0
    exact = representable(want) & exact_mask & ~zero
    loose = ~zero & ~exact
    err = (got - want).abs()
    ulps = err / ulp_bf16(want)
    if not quiet:
        print(f"{what}: exact {int(exact.sum())} (wrong {int((err[exact] != 0).sum())}), one-ulp {int(loose.sum())} "
              f"(worst {ulps[loose].max().item() if loose.any() else 0.0:.3f} ulp), zero {int(zero.sum())} "
              f"(largest {err[zero].max().item() if zero.any() else 0.0:.3g}, allowance up to {tail.max().item():.3g})")
    if not torch.equal(got[exact], want[exact]):
        bad = (exact & (err != 0)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {int(exact.sum())} exact elements differ, first at {i}: "
                             f"got {got[i].item()} want {want[i].item()}")
    if bool((ulps[loose] > 1).any()):
        bad = (loose & (ulps > 1)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} elements off by more than one bf16 ulp (worst {ulps[loose].max().item():.2f}), "
                             f"first at {i}: got {got[i].item()} want {want[i].item()}")
    if bool((err[zero] > tail[zero]).any()):
        bad = (zero & (err > tail)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} elements that should be 0 exceed their allowance, first at {i}: got {got[i].item()}, "
                             f"allowed {tail[i].item():.3g}")


def compare_lse(lse, r, what):
    """|LSE - ideal| < 0.25 / Nkv: a quarter of ln(N / (N - 1)), what one missing key moves it by."""
    err = (lse.detach().double().cpu() - r.lse).abs().max().item()
    assert err < 0.25 / r.Nkv, f"{what}: LSE off by {err}, allowed {0.25 / r.Nkv}"


# ------------------------------------------------------------------ split-query rule of the dK / dV kernel
def dkv_qsplit_py(B, H, Nq, Nkv):
    """Transcription of dkv_qsplit (csrc/attention_v2.hip)."""
    base = (Nkv + 127) // 128 * B * H
    ntiles = (Nq + 63) // 64
    return max(1, min((512 + base - 1) // base, ntiles // 4, 16))


def last_parts(Nq, splits):
    """(number of empty trailing parts, 64-query tiles in the last non-empty part, tiles per part)."""
    ntiles = (Nq + 63) // 64
    per = -(-ntiles // splits)
    used = -(-ntiles // per)
    return splits - used, ntiles - (used - 1) * per, per


def split_count(B, H, Nq, Nkv):
    """The split count the library will use: workspace bytes / (B H Nkv 512), 0 bytes meaning one part."""
    nbytes = _lib.load().gdl_flash_attn_bwd_workspace(B, H, Nq, Nkv)
    assert nbytes % (B * H * Nkv * 512) == 0
    return max(nbytes // (B * H * Nkv * 512), 1)


# (Nq, Nkv, B, H, split count, empty trailing parts, tiles in the last non-empty part / tiles per part)
# Every query has a matching key (Nkv >= 64, or Nq <= Nkv) and no row has more than two (Nkv <= 128): see ideal().
BWD_CASES = [
    (1, 1, 1, 1, 1, 0, (1, 1)), (1, 2, 2, 3, 1, 0, (1, 1)), (31, 33, 1, 8, 1, 0, (1, 1)), (32, 32, 2, 4, 1, 0, (1, 1)),
    (33, 64, 1, 1, 1, 0, (1, 1)), (63, 65, 2, 3, 1, 0, (1, 1)), (64, 127, 1, 8, 1, 0, (1, 1)), (65, 128, 2, 4, 1, 0, (2, 2)),
    (127, 64, 2, 3, 1, 0, (2, 2)), (128, 65, 1, 8, 1, 0, (2, 2)), (129, 127, 2, 4, 1, 0, (3, 3)), (257, 128, 2, 3, 1, 0, (5, 5)),
    (1, 128, 1, 1, 1, 0, (1, 1)), (63, 63, 1, 1, 1, 0, (1, 1)),
    (520, 65, 2, 3, 2, 0, (4, 5)),          # 9 tiles: 5 + 4, the last of them 8 queries
    (777, 127, 1, 8, 3, 0, (3, 5)),         # 13 tiles: 5 + 5 + 3 (short last part)
    (1600, 128, 1, 2, 6, 1, (5, 5)),        # 25 tiles in 6 parts of 5: the sixth is empty
    (1600, 65, 1, 1, 6, 1, (5, 5)),
    (1025, 64, 2, 4, 4, 0, (2, 5)),         # 17 tiles: 5 + 5 + 5 + 2, the last one query
    (4160, 65, 1, 1, 16, 3, (5, 5)),        # 65 tiles in 16 parts of 5: parts 13..15 are empty
    (4160, 128, 1, 2, 16, 3, (5, 5)),
]
BWD_IDS = [f"Nq{c[0]}-Nkv{c[1]}-B{c[2]}H{c[3]}-splits{c[4]}" for c in BWD_CASES]


# ------------------------------------------------------------------ device side: layouts, launchers, kernel selection
def dev(x, dtype=BF16):
    """[B, N, H, 64] float64 -> contiguous [B, N, H * 64] on the GPU."""
    return x.reshape(x.shape[0], x.shape[1], -1).to(DEV, dtype)


def framed(x, left=8, right=8, rows=3, dtype=BF16):
    """A [B, N, D] view of a NaN-filled [B, N + rows, left + D + right] allocation holding x: NaN after the last token
    of every batch (the last one included) and in the channel columns outside the slab."""
    B, N, D = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
    buf = torch.full((B, N + rows, left + D + right), NAN, device=DEV, dtype=dtype)
    view = buf[:, :N, left:left + D]
    view.copy_(dev(x, dtype))
    return buf, view


def nan_frame(B, N, D, left=4, right=12, rows=2):
    buf = torch.full((B, N + rows, left + D + right), NAN, device=DEV, dtype=BF16)
    return buf, buf[:, :N, left:left + D]


def outside_is_nan(buf, view):
    """Everything of `buf` outside `view` (a slice of it) is still NaN, everything inside is finite."""
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    inside.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(True)
    return bool(buf[~inside].isnan().all()) and bool(buf[inside].isfinite().all())


def ptr(t):
    return None if t is None else t.data_ptr()


def fwd_call(q, k, v, H, out, lse):
    """gdl_flash_attn_fwd2 on the caller's buffers (the checked view: an argument error raises ValueError)."""
    B, Nq, Nkv = q.shape[0], q.shape[1], k.shape[1]
    _lib.checked().gdl_flash_attn_fwd2(ptr(q), q.stride(0), q.stride(1), ptr(k), k.stride(0), k.stride(1), ptr(v), v.stride(0),
                                       v.stride(1), ptr(out), out.stride(0), out.stride(1), ptr(lse), B, H, Nq, Nkv, SCALE,
                                       ops._stream())
    torch.cuda.synchronize()


def forward(q, k, v, H):
    """Forward into fresh buffers, LSE NaN-filled before the call."""
    out = torch.full((q.shape[0], q.shape[1], H * HD), NAN, device=DEV, dtype=BF16)
    lse = torch.full((q.shape[0], H, q.shape[1]), NAN, device=DEV, dtype=torch.float32)
    fwd_call(q, k, v, H, out, lse)
    return out, lse


def bwd_call(q, k, v, o, do, lse, dvec, dq, dk, dv, H, ws, ws_bytes):
    B, Nq, Nkv = q.shape[0], q.shape[1], k.shape[1]
    _lib.checked().gdl_flash_attn_bwd(
        ptr(q), q.stride(0), q.stride(1), ptr(k), k.stride(0), k.stride(1), ptr(v), v.stride(0), v.stride(1),
        ptr(o), o.stride(0), o.stride(1), ptr(do), do.stride(0), do.stride(1), ptr(lse), ptr(dvec),
        ptr(dq), dq.stride(0), dq.stride(1), ptr(dk), dk.stride(0), dk.stride(1), ptr(dv), dv.stride(0), dv.stride(1),
        B, H, Nq, Nkv, SCALE, ptr(ws), ws_bytes, ops._stream())
    torch.cuda.synchronize()


def nan_workspace(B, H, Nq, Nkv):
    nbytes = _lib.load().gdl_flash_attn_bwd_workspace(B, H, Nq, Nkv)
    ws = torch.full((nbytes // 4,), NAN, device=DEV, dtype=torch.float32) if nbytes else None
    return ws, nbytes


def backward(q, k, v, o, do, lse, H, dq=None, dk=None, dv=None):
    """Fused backward; dvec and the split-query workspace (exactly the queried size) NaN-filled before the call."""
    B, Nq, Nkv, D = q.shape[0], q.shape[1], k.shape[1], H * HD
    dq = torch.full((B, Nq, D), NAN, device=DEV, dtype=BF16) if dq is None else dq
    dk = torch.full((B, Nkv, D), NAN, device=DEV, dtype=BF16) if dk is None else dk
    dv = torch.full((B, Nkv, D), NAN, device=DEV, dtype=BF16) if dv is None else dv
    dvec = torch.full((B, H, Nq), NAN, device=DEV, dtype=torch.float32)
    ws, nbytes = nan_workspace(B, H, Nq, Nkv)
    bwd_call(q, k, v, o, do, lse, dvec, dq, dk, dv, H, ws, nbytes)
    return dq, dk, dv, dvec


# forward version (gdl_debug_set_flash_fwd) x slack of the deferred maximum; version 2 has no deferred maximum
FORWARD_KERNELS = [(2, 0.0), (2, 6.0), (3, 0.0), (3, 6.0), (4, 0.0), (4, 6.0), (5, 0.0), (5, 6.0)]


@contextlib.contextmanager
def forward_kernel(version, defer):
    lib = _lib.load()
    lib.gdl_debug_set_flash_fwd(version, defer)
    try:
        yield
    finally:
        lib.gdl_debug_set_flash_fwd(-1, 6.0)      # back to the build's default forward


def forward_kernel_name(version, Nq):
    """What gdl_flash_attn_fwd2 launches for `version` (its dispatch, restated: the cases print it)."""
    if version >= 4 and Nq > 64:
        return f"flash_fwd4_kernel<4,{'true' if version == 5 else 'false'}>"
    if version >= 3:
        return f"flash_fwd3_kernel<{4 if Nq > 64 else 2}>"
    return f"flash_fwd2_kernel<{4 if Nq > 128 else 2}>"


# ------------------------------------------------------------------ shapes
# (Nq, Nkv, B, H): every edge value of Nq and of Nkv with a small and with a large partner; 64 queries (the two-wave
# flash_fwd3_kernel), 128 queries (the nw choice of flash_fwd2_kernel), 65 / 129 / 257 queries (blocks whose trailing waves
# are idle); B H = 8 and B H = 6 both with one and with several query blocks (the two orders of decode_block)
SHAPES = [
    (1, 1, 1, 1), (1, 193, 2, 3), (1, 65, 1, 8), (31, 2, 2, 4), (31, 129, 1, 1), (32, 31, 2, 3), (32, 191, 1, 8),
    (33, 32, 2, 4), (33, 128, 1, 1), (63, 33, 2, 3), (63, 127, 1, 8), (64, 63, 2, 4), (64, 64, 1, 1), (64, 193, 2, 3),
    (65, 1, 1, 8), (65, 65, 2, 4), (127, 2, 1, 1), (127, 193, 2, 3), (128, 31, 1, 8), (128, 128, 2, 4), (129, 32, 1, 1),
    (129, 129, 2, 3), (127, 127, 1, 8), (257, 1, 1, 8), (257, 33, 2, 3), (257, 63, 2, 4), (257, 64, 2, 3), (257, 65, 1, 1), (257, 191, 1, 8), (257, 193, 2, 4),
]
SHAPE_IDS = [f"Nq{a}-Nkv{b}-B{c}H{d}" for a, b, c, d in SHAPES]
OTHER_SHAPES = [s for s in SHAPES if s[:2] in ((1, 193), (31, 2), (33, 32), (63, 127), (64, 64), (65, 65), (128, 31),
                                               (129, 129), (257, 63), (257, 193))]
OTHER_IDS = [f"Nq{a}-Nkv{b}-B{c}H{d}" for a, b, c, d in OTHER_SHAPES]
# (Nq, Nkv, B, H, position of the dominant key)
DOMINANT = [(65, 193, 2, 3, p) for p in (192, 191, 0, 31, 32, 63, 64)] + [(33, 65, 1, 8, 64), (129, 64, 2, 4, 63),
                                                                          (64, 33, 1, 1, 32), (1, 2, 2, 3, 1)]


def test_shape_list_covers_the_edges():
    nq, nkv = {s[0] for s in SHAPES}, {s[1] for s in SHAPES}
    assert nq == {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257} and nkv == {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193}
    for n in nq:
        partners = [s[1] for s in SHAPES if s[0] == n]
        assert min(partners) <= 64 <= max(partners), n
    for n in nkv:
        partners = [s[0] for s in SHAPES if s[1] == n]
        assert min(partners) <= 65 <= max(partners), n
    assert {(s[2], s[3]) for s in SHAPES} == {(1, 1), (2, 3), (1, 8), (2, 4)}
    for bh8 in (True, False):      # both orders of decode_block, each with more than one query block of 128
        assert any(((s[2] * s[3]) % 8 == 0) == bh8 and s[0] > 128 for s in SHAPES)


# ------------------------------------------------------------------ families 1-3 on every forward kernel
def run_forward_family(inputs, shape, what, exact=None):
    Nq, Nkv, B, H = shape[:4]
    q, k, v = inputs
    r = ideal(q, k, v)
    qd, kd, vd = dev(q), dev(k), dev(v)
    for version, defer in FORWARD_KERNELS:
        with forward_kernel(version, defer):
            out, lse = forward(qd, kd, vd, H)
        tag = f"{what} {shape} {forward_kernel_name(version, Nq)} defer {defer}"
        compare(out, r.o, r.pow2 if exact is None else exact, r.a_o, tag, quiet=(version, defer) != (3, 6.0))
        compare_lse(lse, r, tag)
    return r


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_uniform_attention_counts_every_key_once(shape):
    """Family 1: O[b, q, h, d] = w(b, h) * (weighted count of the keys j = d mod 64) / Nkv, LSE = ln Nkv.  Exact where Nkv is
    a power of two; otherwise one bf16 ulp: the kernel multiplies the exact f32 sum by fl(1 / Nkv) and rounds the product to
    bf16, two roundings where the ideal value has one.  Channels without a key (d >= Nkv) are exactly 0."""
    Nq, Nkv, B, H = shape
    r = run_forward_family(uniform_inputs(B, H, Nq, Nkv), shape, "uniform")
    assert r.tail_o == 0.0 and bool((r.c == Nkv).all())


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_heads_and_batches_are_routed(shape):
    """Family 2: the output of (b, h) is the integer 1 + b H + h, bit for bit, for every Nkv: the f32 sum id * Nkv is exact,
    fl(1 / Nkv) is within 2^-24 of 1 / Nkv, and the product, within 2^-23 of the bf16 number id, rounds to it."""
    Nq, Nkv, B, H = shape
    run_forward_family(routing_inputs(B, H, Nq, Nkv), shape, "routing", exact=True)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_hard_selection_addresses_every_key(shape):
    """Family 3: query i returns the mean of the V rows j = i mod 64 (for Nkv <= 64 the row itself, bit for bit; a query
    without a matching key the mean of all rows).  Exact where the number of averaged rows is a power of two; otherwise one
    bf16 ulp for the same reason as in family 1 (fl(1 / c), then the bf16 rounding of the product)."""
    Nq, Nkv, B, H = shape
    r = run_forward_family(selection_inputs(B, H, Nq, Nkv), shape, "selection")
    if Nkv <= 64:
        _, _, v = selection_inputs(B, H, Nq, Nkv)
        rows = torch.arange(Nq)[torch.arange(Nq) % 64 < Nkv]
        assert torch.equal(r.o[:, rows], v[:, rows % 64]) and bool(r.pow2[:, rows].all())


@pytest.mark.parametrize("case", DOMINANT, ids=[f"Nq{a}-Nkv{b}-B{c}H{d}-at{p}" for a, b, c, d, p in DOMINANT])
def test_dominant_key_is_selected_at_every_position(case):
    """Family 3 with one key that scores 64 with every query (32 above the matching keys): every query returns that key's V
    row bit for bit -- at the very last position behind the masked tail of the last tile, at the tile edges, and after
    tiles whose maximum was kept (the deferred kernels rescale by e^-32 when they meet it)."""
    Nq, Nkv, B, H, pos = case
    q, k, v = selection_inputs(B, H, Nq, Nkv, dominant=pos)
    r = run_forward_family((q, k, v), case, "dominant", exact=True)
    assert torch.equal(r.o, v[:, pos:pos + 1].expand(B, Nq, H, HD)) and bool((r.lse == 64.0).all())


# ------------------------------------------------------------------ families 1-3 on the v1 and the unfused forward
def other_paths():
    return {"v1-bf16": (ops.attention_flash_v1, BF16), "unfused-bf16": (ops.attention_unfused, BF16),
            "unfused-f32": (ops.attention_unfused, torch.float32)}


@pytest.mark.parametrize("shape", OTHER_SHAPES, ids=OTHER_IDS)
@pytest.mark.parametrize("path", ["v1-bf16", "unfused-bf16", "unfused-f32"])
def test_v1_and_unfused_forward(path, shape):
    """Families 1-3 and a dominant last key on ops.attention_flash_v1 and ops.attention_unfused (bf16, and f32 for the latter),
    same per-element criteria.  The unfused bf16 path materialises P in bf16: bf16(1 / c) is 1 / c only for c a power of two,
    so the routing family, bit-exact on the fused kernels, is held to one bf16 ulp there unless Nkv is a power of two (c
    bf16(1 / c) id is within 2^-9 of id before its own rounding).  The f32 path claims no exactness at all: its softmax
    rounds 1 / c to f32 and its GEMM rounds every one of up to 193 partial sums (the integer 1 comes back as 1.000002, 17 f32
    ulps), so one f32 ulp is not attainable either; every non-zero element is held to one bf16 ulp of its own value, the
    criterion of the other paths, and a zero element to its allowance."""
    Nq, Nkv, B, H = shape
    fn, dtype = other_paths()[path]
    families = {"uniform": (uniform_inputs(B, H, Nq, Nkv), None), "routing": (routing_inputs(B, H, Nq, Nkv), None),
                "selection": (selection_inputs(B, H, Nq, Nkv), None),
                "dominant": (selection_inputs(B, H, Nq, Nkv, dominant=Nkv - 1), None)}
    if path == "unfused-f32":
        families = {name: (inputs, False) for name, (inputs, _) in families.items()}
    elif path == "v1-bf16":
        families["routing"] = (families["routing"][0], True)
    for name, ((q, k, v), exact) in families.items():
        r = ideal(q, k, v)
        out = fn(dev(q, dtype), dev(k, dtype), dev(v, dtype), H)
        torch.cuda.synchronize()
        compare(out, r.o, r.pow2 if exact is None else exact, r.a_o, f"{path} {name} {shape}")


# ------------------------------------------------------------------ family 4: the backward
@functools.lru_cache(maxsize=None)
def backward_problem(Nq, Nkv, B, H):
    q, k, v = selection_inputs(B, H, Nq, Nkv, signed=True)
    do = grad_output(B, H, Nq)
    return q, k, v, do, ideal(q, k, v, do)


def check_gradients(got, r, what):
    """dQ, dK, dV (and dvec) against the ideal gradients.  P, dS and O round to bf16 exactly (asserted in ideal()) and every f32
    sum is exact, so an element whose ideal value is a bf16 number is bit-equal; one that needs more than 8 bits is within
    one bf16 ulp -- the final f32 -> bf16 store is its one rounding, and an exact tie may fall either way once the e^-32 tail is
    in the accumulator."""
    for name, g, want, allow in (("dq", got[0], r.dq, r.a_dq), ("dk", got[1], r.dk, r.a_dk), ("dv", got[2], r.dv, r.a_dv)):
        compare(g, want, True, allow, f"{what} {name}")
    if len(got) > 3:       # f32: the exact sum of dyadic numbers plus whatever the zero elements of O carry
        err = (got[3].detach().double().cpu() - r.dvec).abs()
        print(f"{what} dvec: largest error {err.max().item():.3g}, allowance up to {r.a_dvec.max().item():.3g}")
        assert bool((err <= r.a_dvec).all()), f"{what} dvec"


@pytest.mark.parametrize("case", BWD_CASES, ids=BWD_IDS)
def test_fused_backward_exact(case):
    """Family 4 through gdl_flash_attn_bwd: o and lse from the forward, a NaN-filled workspace of the queried size; the
    split count (which reduction ran: direct stores, or f32 partials + flash_bwd_dkv_reduce_kernel), the empty trailing
    parts and the short last part are asserted per case."""
    Nq, Nkv, B, H, want_splits, want_empty, want_last = case
    q, k, v, do, r = backward_problem(Nq, Nkv, B, H)
    splits = split_count(B, H, Nq, Nkv)
    empty, last, per = last_parts(Nq, splits)
    what = f"fused bwd Nq {Nq} Nkv {Nkv} B {B} H {H}: {splits} parts of {per} tiles, {empty} empty, last holds {last}"
    assert splits == want_splits == dkv_qsplit_py(B, H, Nq, Nkv), f"{what}: designed for {want_splits}"
    assert (empty, (last, per)) == (want_empty, want_last), what
    qd, kd, vd, dod = dev(q), dev(k), dev(v), dev(do)
    o, lse = forward(qd, kd, vd, H)
    compare(o, r.o, True, r.a_o, f"{what} o")
    compare_lse(lse, r, what)
    check_gradients(backward(qd, kd, vd, o, dod, lse, H), r, what)


@pytest.mark.parametrize("case", [c for c in BWD_CASES if c[0] <= 777], ids=[i for c, i in zip(BWD_CASES, BWD_IDS) if c[0] <= 777])
def test_backward_through_ops(case):
    """The same inputs through ops.attention_bwd: with o / lse (the fused kernels behind the wrapper's own workspace) and
    without (the materialised backward: bf16 P and dS in HBM, batched GEMMs and weight-gradient kernels)."""
    Nq, Nkv, B, H = case[:4]
    q, k, v, do, r = backward_problem(Nq, Nkv, B, H)
    qd, kd, vd, dod = dev(q), dev(k), dev(v), dev(do)
    o, lse = ops.attention_flash(qd, kd, vd, H, return_lse=True)
    for tag, extra in (("ops fused", dict(o=o, lse=lse)), ("ops materialised", {})):
        dq, dk, dv = (torch.full_like(t, NAN) for t in (qd, kd, vd))
        ops.attention_bwd(qd, kd, vd, dod, H, dq, dk, dv, **extra)
        torch.cuda.synchronize()
        check_gradients((dq, dk, dv), r, f"{tag} {case[:4]}")


# ------------------------------------------------------------------ family 5: poisoned surroundings
POISON = [(63, 63, 2, 3), (33, 128, 1, 8), (520, 65, 2, 3)]      # a masked last key tile; ...; two query parts


@pytest.mark.parametrize("shape", POISON, ids=[f"Nq{a}-Nkv{b}-B{c}H{d}" for a, b, c, d in POISON])
def test_poisoned_surroundings(shape):
    """q, k, v, o, dO as views of larger NaN-filled allocations (NaN token rows behind the last token of every batch, NaN
    channel columns beside the H * 64 slab); out, dq, dk, dv as slices of NaN-filled packed buffers; lse, dvec and the
    workspace NaN-filled.  Results are bit-identical to the clean run and nothing outside the slices is written."""
    Nq, Nkv, B, H = shape
    D = H * HD
    q, k, v, do, r = backward_problem(Nq, Nkv, B, H)
    clean = [dev(t) for t in (q, k, v, do)]
    framed_in = [framed(t)[1] for t in (q, k, v, do)]
    for version, defer in FORWARD_KERNELS:
        with forward_kernel(version, defer):
            o0, lse0 = forward(*clean[:3], H)
            obuf, o1 = nan_frame(B, Nq, D)
            lse1 = torch.full_like(lse0, NAN)
            fwd_call(*framed_in[:3], H, o1, lse1)
        tag = f"poisoned forward {shape} version {version} defer {defer}"
        assert outside_is_nan(obuf, o1), f"{tag}: wrote outside its slice, or NaN inside"
        assert torch.equal(o1, o0) and torch.equal(lse1, lse0), f"{tag}: differs from the clean run"
    compare(o0, r.o, True, r.a_o, f"poisoned forward {shape} o")
    g0 = backward(*clean[:3], o0, clean[3], lse0, H)
    obuf, o_in = nan_frame(B, Nq, D, left=8, right=8)
    o_in.copy_(o0)
    frames = [nan_frame(B, n, D) for n in (Nq, Nkv, Nkv)]
    g1 = backward(*framed_in[:3], o_in, framed_in[3], lse0, H, *(f[1] for f in frames))
    for name, a, b_, (buf, view) in zip(("dq", "dk", "dv"), g0, g1, frames):
        assert outside_is_nan(buf, view), f"poisoned backward {shape}: {name} wrote outside its slice, or NaN inside"
        assert torch.equal(a, b_), f"poisoned backward {shape}: {name} differs from the clean run"
    assert torch.equal(g0[3], g1[3]) and bool(g1[3].isfinite().all())
    check_gradients(g1, r, f"poisoned backward {shape}")


def test_misaligned_calls_are_refused_before_any_launch():
    """A token stride that is no multiple of 8 elements, an input pointer off 16 bytes, a missing / too small workspace for a
    split backward: the binding's argument error (ValueError), and every NaN-filled output is still NaN afterwards."""
    Nq, Nkv, B, H = 520, 65, 2, 3
    D = H * HD
    q, k, v, do, _ = backward_problem(Nq, Nkv, B, H)
    qd, kd, vd, dod = (dev(t) for t in (q, k, v, do))
    o, lse = forward(qd, kd, vd, H)
    assert split_count(B, H, Nq, Nkv) == 2
    k_odd_stride = framed(k, left=8, right=4)[1]           # token stride 204
    q_off = framed(q, left=4, right=4)[1]                  # pointer 8 bytes off, strides fine
    do_odd_stride = framed(do, left=8, right=4)[1]
    assert k_odd_stride.stride(1) % 8 != 0 and q_off.data_ptr() % 16 == 8 and q_off.stride(1) % 8 == 0 and q_off.stride(0) % 8 == 0

    def untouched(*ts):
        torch.cuda.synchronize()
        return all(bool(t.isnan().all()) for t in ts)

    for tag, (qq, kk) in {"k token stride": (qd, k_odd_stride), "q pointer": (q_off, kd)}.items():
        out, l = torch.full_like(qd, NAN), torch.full_like(lse, NAN)
        with pytest.raises(ValueError, match="gdl_flash_attn_fwd2"):
            fwd_call(qq, kk, vd, H, out, l)
        assert untouched(out, l), f"forward, {tag}: something ran"
    ws, nbytes = nan_workspace(B, H, Nq, Nkv)
    bad = {"dO token stride": dict(do=do_odd_stride), "q pointer": dict(q=q_off), "no workspace": dict(ws=None, ws_bytes=0),
           "workspace 4 bytes short": dict(ws_bytes=nbytes - 4)}
    ws_big = torch.full((nbytes // 4 + 1,), NAN, device=DEV, dtype=torch.float32)
    bad["workspace pointer 4 bytes off"] = dict(ws=ws_big[1:], ws_bytes=nbytes)
    for tag, change in bad.items():
        outs = [torch.full_like(t, NAN) for t in (qd, kd, vd)]
        dvec = torch.full_like(lse, NAN)
        a = dict(q=qd, k=kd, v=vd, o=o, do=dod, lse=lse, dvec=dvec, dq=outs[0], dk=outs[1], dv=outs[2], H=H, ws=ws, ws_bytes=nbytes)
        a.update(change)
        with pytest.raises(ValueError, match="gdl_flash_attn_bwd"):
            bwd_call(**a)
        assert untouched(*outs, dvec, ws), f"backward, {tag}: something ran"
