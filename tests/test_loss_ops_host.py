"""What every loss wrapper of gdlhip.ops hands to its C entry point, pinned without a GPU or a library: the symbol, the argument
count and ctypes kinds of ``_lib.SIGNATURES``, and every value position by position (dims, the options' ``c_args()`` run,
``grad_scale``, ``accumulate``, the ``form`` tag, the workspace bytes the fake ``*_workspace`` returned, the stream last).  The
Dice / Jaccard / Tversky family has the same in tests/test_overlap_loss_host.py and tests/test_binary_lowres_host.py.

The dimensions are pairwise distinct (B=2, K=3, 4x5 -> 8x10), so a swapped pair cannot pass."""

import ctypes as C

import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import _lib  # noqa: E402
from gdlhip import ops  # noqa: E402

B, K, HI, WI, HO, WO = 2, 3, 4, 5, 8, 10
HW = HO * WO
NCHW, LOW, BIN = (B, K, HW), (B, K, HI, WI, HO, WO), (B, HI, WI, HO, WO)
GS, WS, STREAM = 0.25, 4168, 7      # grad_scale, the bytes every fake *_workspace answers, the fake stream
ANY = object()                       # a non-null pointer to a buffer the wrapper allocated itself

X, LOWK = torch.zeros(B, K, HO, WO), torch.zeros(B, HI, WI, K)
X1, LOW1 = torch.zeros(B, 1, HO, WO), torch.zeros(B, HI, WI, 1)
Y, YF = torch.zeros(B, HO, WO, dtype=torch.int64), torch.zeros(B, HO, WO)
Y1, YK = torch.zeros(B, 1, HO, WO, dtype=torch.int64), torch.zeros(B, K, HO, WO)
UP, NORM, NORM1, NORMK = torch.ones(()), torch.ones(1), torch.ones(B), torch.ones(B * K)
COEF, COEF1 = torch.zeros(X.numel()), torch.zeros(X1.numel())
OUT, OUT1 = torch.zeros_like(X), torch.zeros_like(X1)
STATE = torch.zeros(11, dtype=torch.float64)

SCE = ops.SoftCEOptions(0.125, 255, False)
FOC = ops.FocalOptions(1.5, 0.375, 255, True, 0.75)
XENT = ops.CrossEntropyOptions(0.125, 255, True, torch.ones(K))
BCE = ops.SoftBCEOptions(0.125, 255, True, torch.ones(1), torch.full((1,), 1.5))
BCEK = ops.SoftBCEOptions(None, None, False, torch.ones(K), None)
LOV, LOVI = ops.LovaszOptions(False, 255), ops.LovaszOptions(True, None)
TILE, GATHER, AUTO = _lib.FOCAL_TILE, _lib.FOCAL_GATHER, _lib.FOCAL_AUTO
I64, F32T = _lib.BCE_TARGET_I64, _lib.BCE_TARGET_F32


def test_the_option_runs_are_what_the_cases_below_expect():
    assert SCE.c_args() == (0.125, 1, 255, 0)
    assert FOC.c_args() == (1.5, 1, 0.375, 1, 0.75, 1, 255, 1)
    assert XENT.c_args()[1:] == (0.125, 1, 255, 1) and XENT.c_args()[0].value == XENT.weight.data_ptr()
    assert LOV.c_args() == (0, 1, 255) and LOVI.c_args() == (1, 0, 0)
    got = BCE.c_args(160)
    assert got[:5] == (1, 0.125, 1, 255, 255.0) and got[5].value == BCE.weight.data_ptr() and got[6] == 1
    assert got[7].value == BCE.pos_weight.data_ptr() and got[8:] == (1, 1.0 / 160)
    got = BCEK.c_args(160)
    assert got[:5] == (0, 0.0, 0, 0, 0.0) and got[5].value == BCEK.weight.data_ptr() and got[6:] == (K, None, 0, 1.0)


# id, the call, the symbol, the arguments it must receive in front of the stream, the *_workspace / *_state calls it must make
CASES = [
    ("soft_ce_fwd", lambda: ops.soft_ce_fwd(X, Y, SCE), "gdl_soft_ce_fwd",
     [X, Y, *NCHW, *SCE.c_args(), ANY, ANY, WS], [("gdl_soft_ce_workspace", NCHW)]),
    ("soft_ce_bwd", lambda: ops.soft_ce_bwd(X, Y, UP, GS, SCE, OUT, True), "gdl_soft_ce_bwd",
     [X, Y, *NCHW, *SCE.c_args(), UP, GS, OUT, 1], []),
    ("soft_ce_bwd-own-out", lambda: ops.soft_ce_bwd(X, Y, UP, GS, SCE), "gdl_soft_ce_bwd",
     [X, Y, *NCHW, *SCE.c_args(), UP, GS, ANY, 0], []),
    ("soft_ce_lowres_fwd", lambda: ops.soft_ce_lowres_fwd(LOWK, Y, (HO, WO), SCE), "gdl_soft_ce_lowres_fwd",
     [LOWK, Y, *LOW, *SCE.c_args(), ANY, ANY, WS], [("gdl_soft_ce_lowres_workspace", (B, K, HO, WO))]),
    ("soft_ce_lowres_fwd-fused", lambda: ops.soft_ce_lowres_fwd(LOWK, Y, (HO, WO), SCE, fused=True), "gdl_soft_ce_lowres_fused_fwd",
     [LOWK, Y, *LOW, *SCE.c_args(), ANY, ANY, (WS // 8 + 1) * 8], [("gdl_soft_ce_lowres_fused_state", LOW)]),
    ("soft_ce_lowres_bwd", lambda: ops.soft_ce_lowres_bwd(LOWK, Y, (HO, WO), UP, GS, SCE), "gdl_soft_ce_lowres_bwd",
     [LOWK, Y, *LOW, *SCE.c_args(), UP, GS, ANY, ANY, WS], [("gdl_soft_ce_lowres_bwd_workspace", LOW)]),
    ("soft_ce_lowres_bwd-fused", lambda: ops.soft_ce_lowres_bwd(LOWK, Y, (HO, WO), UP, GS, SCE, state=STATE),
     "gdl_soft_ce_lowres_fused_bwd", [STATE, STATE.numel() * 8, *LOW, 0, UP, GS, ANY], []),
    ("focal_fwd", lambda: ops.focal_fwd(X, Y, FOC), "gdl_focal_fwd",
     [X, Y, *NCHW, *FOC.c_args(), ANY, ANY, ANY, WS], [("gdl_focal_workspace", NCHW)]),
    ("focal_bwd", lambda: ops.focal_bwd(X, Y, NORM, UP, GS, FOC, OUT, True), "gdl_focal_bwd",
     [X, Y, *NCHW, *FOC.c_args(), NORM, UP, GS, OUT, 1], []),
    ("focal_binary_fwd", lambda: ops.focal_binary_fwd(X1, Y1, FOC), "gdl_focal_binary_fwd",
     [X1, Y1, B * HW, *FOC.c_args(), ANY, ANY, ANY, WS], [("gdl_focal_workspace", (1, 1, B * HW))]),
    ("focal_binary_bwd", lambda: ops.focal_binary_bwd(X1, Y1, NORM, UP, GS, FOC, OUT1, True), "gdl_focal_binary_bwd",
     [X1, Y1, B * HW, *FOC.c_args(), NORM, UP, GS, OUT1, 1], []),
    ("focal_lowres_fwd", lambda: ops.focal_lowres_fwd(LOWK, Y, (HO, WO), FOC), "gdl_focal_lowres_fwd",
     [LOWK, Y, *LOW, *FOC.c_args(), ANY, ANY, ANY, WS], [("gdl_focal_lowres_workspace", (B, K, HO, WO))]),
    ("focal_lowres_bwd-tile", lambda: ops.focal_lowres_bwd(LOWK, Y, (HO, WO), NORM, UP, GS, FOC, form="tile"), "gdl_focal_lowres_bwd",
     [LOWK, Y, *LOW, *FOC.c_args(), NORM, UP, GS, ANY, ANY, WS, TILE], [("gdl_focal_lowres_bwd_workspace", LOW)]),
    ("focal_lowres_bwd-gather", lambda: ops.focal_lowres_bwd(LOWK, Y, (HO, WO), NORM, UP, GS, FOC, form="gather"), "gdl_focal_lowres_bwd",
     [LOWK, Y, *LOW, *FOC.c_args(), NORM, UP, GS, ANY, None, 0, GATHER], []),
    ("focal_binary_lowres_fwd", lambda: ops.focal_binary_lowres_fwd(LOW1, Y, (HO, WO), FOC), "gdl_focal_binary_lowres_fwd",
     [LOW1, Y, *BIN, *FOC.c_args(), ANY, ANY, ANY, WS], [("gdl_focal_lowres_workspace", (B, 1, HO, WO))]),
    ("focal_binary_lowres_bwd-tile", lambda: ops.focal_binary_lowres_bwd(LOW1, Y, (HO, WO), NORM, UP, GS, FOC, form="tile"),
     "gdl_focal_binary_lowres_bwd", [LOW1, Y, *BIN, *FOC.c_args(), NORM, UP, GS, ANY, ANY, WS, TILE],
     [("gdl_binary_lowres_bwd_workspace", BIN)]),
    ("focal_binary_lowres_bwd-gather", lambda: ops.focal_binary_lowres_bwd(LOW1, Y, (HO, WO), NORM, UP, GS, FOC, form="gather"),
     "gdl_focal_binary_lowres_bwd", [LOW1, Y, *BIN, *FOC.c_args(), NORM, UP, GS, ANY, None, 0, GATHER], []),
    ("cross_entropy_fwd", lambda: ops.cross_entropy_fwd(X, Y, XENT), "gdl_cross_entropy_fwd",
     [X, Y, *NCHW, *XENT.c_args(), ANY, ANY, ANY, WS], [("gdl_cross_entropy_workspace", NCHW)]),
    ("cross_entropy_bwd", lambda: ops.cross_entropy_bwd(X, Y, NORM, UP, GS, XENT, OUT, True), "gdl_cross_entropy_bwd",
     [X, Y, *NCHW, *XENT.c_args(), NORM, UP, GS, OUT, 1], []),
    ("cross_entropy_lowres_fwd", lambda: ops.cross_entropy_lowres_fwd(LOWK, Y, (HO, WO), XENT), "gdl_cross_entropy_lowres_fwd",
     [LOWK, Y, *LOW, *XENT.c_args(), ANY, ANY, ANY, WS], [("gdl_cross_entropy_lowres_workspace", (B, K, HO, WO))]),
    ("cross_entropy_lowres_bwd-auto", lambda: ops.cross_entropy_lowres_bwd(LOWK, Y, (HO, WO), NORM, UP, GS, XENT),
     "gdl_cross_entropy_lowres_bwd", [LOWK, Y, *LOW, *XENT.c_args(), NORM, UP, GS, ANY, ANY, WS, AUTO],
     [("gdl_cross_entropy_lowres_bwd_workspace", LOW)]),
    ("cross_entropy_lowres_bwd-gather", lambda: ops.cross_entropy_lowres_bwd(LOWK, Y, (HO, WO), NORM, UP, GS, XENT, form="gather"),
     "gdl_cross_entropy_lowres_bwd", [LOWK, Y, *LOW, *XENT.c_args(), NORM, UP, GS, ANY, None, 0, GATHER], []),
    ("soft_bce_fwd", lambda: ops.soft_bce_fwd(X, YK, BCEK), "gdl_soft_bce_fwd",
     [X, YK, F32T, *NCHW, *BCEK.c_args(X.numel()), ANY, ANY, WS], [("gdl_soft_bce_workspace", NCHW)]),
    ("soft_bce_bwd", lambda: ops.soft_bce_bwd(X1, Y, UP, GS, BCE, OUT1, True), "gdl_soft_bce_bwd",
     [X1, Y, I64, B, 1, HW, *BCE.c_args(X1.numel()), UP, GS, OUT1, 1], []),
    ("soft_bce_lowres_fwd", lambda: ops.soft_bce_lowres_fwd(LOW1, YF, (HO, WO), BCE), "gdl_soft_bce_lowres_fwd",
     [LOW1, YF, F32T, *BIN, *BCE.c_args(B * HW), ANY, ANY, WS], [("gdl_soft_bce_lowres_workspace", (B, HO, WO))]),
    ("soft_bce_lowres_bwd-tile", lambda: ops.soft_bce_lowres_bwd(LOW1, Y, (HO, WO), UP, GS, BCE, form="tile"), "gdl_soft_bce_lowres_bwd",
     [LOW1, Y, I64, *BIN, *BCE.c_args(B * HW), UP, GS, ANY, ANY, WS, TILE], [("gdl_binary_lowres_bwd_workspace", BIN)]),
    ("soft_bce_lowres_bwd-gather", lambda: ops.soft_bce_lowres_bwd(LOW1, Y, (HO, WO), UP, GS, BCE, form="gather"),
     "gdl_soft_bce_lowres_bwd", [LOW1, Y, I64, *BIN, *BCE.c_args(B * HW), UP, GS, ANY, None, 0, GATHER], []),
    ("lovasz_fwd", lambda: ops.lovasz_fwd(X, Y, LOV), "gdl_lovasz_fwd",
     [X, Y, *NCHW, *LOV.c_args(), ANY, ANY, ANY, ANY, WS], [("gdl_lovasz_workspace", (K, B * HW, K))]),
    ("lovasz_fwd-per-image", lambda: ops.lovasz_fwd(X, Y, LOVI), "gdl_lovasz_fwd",
     [X, Y, *NCHW, *LOVI.c_args(), ANY, ANY, ANY, ANY, WS], [("gdl_lovasz_workspace", (B * K, HW, K))]),
    ("lovasz_bwd", lambda: ops.lovasz_bwd(X, Y, COEF, NORMK, UP, GS, LOVI, OUT, True), "gdl_lovasz_bwd",
     [X, Y, *NCHW, *LOVI.c_args(), COEF, NORMK, UP, GS, OUT, 1], []),
    ("lovasz_binary_fwd", lambda: ops.lovasz_binary_fwd(X1, Y1, LOVI), "gdl_lovasz_binary_fwd",
     [X1, Y1, B, HW, *LOVI.c_args(), ANY, ANY, ANY, ANY, WS], [("gdl_lovasz_workspace", (B, HW, 1))]),
    ("lovasz_binary_bwd", lambda: ops.lovasz_binary_bwd(X1, Y1, COEF1, NORM, UP, GS, LOV, OUT1, True), "gdl_lovasz_binary_bwd",
     [X1, Y1, B, HW, *LOV.c_args(), COEF1, NORM, UP, GS, OUT1, 1], []),
]


def _matches(got, want) -> bool:
    if want is ANY:
        return isinstance(got, C.c_void_p) and bool(got.value)
    if want is None:
        return got is None
    if isinstance(want, torch.Tensor):
        return isinstance(got, C.c_void_p) and got.value == want.data_ptr()
    if isinstance(want, C.c_void_p):
        return isinstance(got, C.c_void_p) and got.value == want.value
    return type(got) is type(want) and got == want


def _kind_ok(value, ctype) -> bool:
    if ctype is C.c_float:
        return type(value) is float
    if ctype in (C.c_int, C.c_int64):
        return type(value) is int
    assert ctype is C.c_void_p, ctype
    return value is None or type(value) in (int, C.c_void_p)


@pytest.mark.parametrize("call,symbol,want,sized", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_wrapper_hands_the_entry_point_its_arguments_in_order(monkeypatch, call, symbol, want, sized):
    calls, sizes = [], []

    class Recorder:
        """Either view of the library: a size query may go through both, a launch only through the one that checks its status."""

        def __init__(self, checks_status):
            self.checks_status = checks_status

        def __getattr__(self, name):
            if name.endswith("_workspace") or name.endswith("_state"):
                return lambda *a: sizes.append((name, a)) or WS
            assert self.checks_status and name in _lib.STATUS_FUNCTIONS, f"{name}: launched through the view that drops its status"
            return lambda *a: calls.append((name, a)) or 0

    monkeypatch.setattr(_lib, "load", lambda: Recorder(False))
    monkeypatch.setattr(_lib, "checked", lambda: Recorder(True))
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    call()
    assert [c[0] for c in calls] == [symbol]
    assert sizes == sized
    args, types = calls[0][1], _lib.SIGNATURES[symbol][1]
    assert len(args) == len(types)
    for i, (a, t) in enumerate(zip(args, types)):
        assert _kind_ok(a, t), (symbol, i, a, t)
    assert args[-1] == STREAM
    assert len(want) == len(args) - 1
    for i, (a, w) in enumerate(zip(args, want)):
        assert _matches(a, w), (symbol, i, a, w)


def test_a_fused_soft_ce_forward_the_shape_does_not_take_runs_the_plain_one(monkeypatch):
    """``gdl_soft_ce_lowres_fused_state`` answering 0: the plain forward and ``state`` None."""
    calls = []

    class Recorder:
        def __getattr__(self, name):
            if name.endswith("_state"):
                return lambda *a: 0
            if name.endswith("_workspace"):
                return lambda *a: WS
            return lambda *a: calls.append(name) or 0

    monkeypatch.setattr(_lib, "load", lambda: Recorder())
    monkeypatch.setattr(_lib, "checked", lambda: Recorder())
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    loss, state = ops.soft_ce_lowres_fwd(LOWK, Y, (HO, WO), SCE, fused=True)
    assert calls == ["gdl_soft_ce_lowres_fwd"] and state is None and loss.shape == ()


def test_the_lowres_predicates_are_one_function_under_four_names():
    ok, no = torch.zeros(1, 2, 2, 16), torch.zeros(1, 2, 2, 17)
    for f in (ops.dice_lowres_ok, ops.soft_ce_lowres_ok, ops.focal_lowres_ok, ops.cross_entropy_lowres_ok):
        assert f(ok, (128, 128)) and not f(no, (128, 128)) and not f(ok, (129, 128)) and not f(ok, (1, 2)) and not f(ok[0], (4, 4))
