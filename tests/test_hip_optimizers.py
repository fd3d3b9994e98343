"""GPU tests of gdlhip.nn.FusedAdamW / FusedSGD: parity with torch.optim.AdamW / SGD + clip_grad_norm_, the machinery they share
with FusedAdam (chunk-table reuse, bf16 operand shadows, capturable form), the hipGraph-captured step against an all-eager
twin (own process per scenario: tests/_optimizer_graph_worker.py) and the MiniTrainer wiring with a checkpoint round trip.

Parity bound (per parameter): 4 x the largest deviation of torch's OWN f32 CPU run from torch's f64 run on the same f32 inputs,
with a floor of 2 f32 ulp of the parameter's largest magnitude.  Reference against reference: the code under test never enters the
bound.  The factor 4 covers the kernels' operation order (lr / bc1 and rsqrt(bc2) as step-wide scalars, the f32 global norm).

Bit-for-bit comparisons (tests 2, 5, 6, 7) run WITHOUT the global-norm clip: its reduction adds the per-chunk sums with float
atomics, so the clip coefficient may differ in its last bit between two runs of the very same code; the clip itself is held
to torch's by the parity tests."""

import json
import os
import subprocess
import sys
from functools import partial
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip import ops  # noqa: E402

DEV = "cuda"

# [1]; exactly one chunk; two chunks, the second with one element; 2-d; channels_last conv; one parameter without a gradient
SHAPES = [(1,), (65536,), (65537,), (1000, 3), (64, 32, 3, 3), (7,)]
GROUP_A, GROUP_B, NO_GRAD = (0, 1, 3), (2, 4, 5), 5

ADAMW = ("adamw", dict(lr=1e-3, weight_decay=1e-2), dict(lr=3e-4, weight_decay=0.1))
SGD_CASES = [
    ("plain", dict(lr=0.1), dict(lr=0.03, weight_decay=5e-3)),
    ("momentum", dict(lr=0.1, momentum=0.9), dict(lr=0.03, weight_decay=5e-3, momentum=0.0)),
    ("dampening", dict(lr=0.1, momentum=0.9, dampening=0.5), dict(lr=0.03, weight_decay=5e-3, momentum=0.5)),
    ("nesterov", dict(lr=0.1, momentum=0.9, nesterov=True), dict(lr=0.03, weight_decay=5e-3, momentum=0.5)),
    ("weight_decay", dict(lr=0.1, weight_decay=1e-2), dict(lr=0.03, weight_decay=5e-3, momentum=0.9)),
]


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    ps[4] = ps[4].contiguous(memory_format=torch.channels_last)
    gs = [torch.randn(s, generator=g) * 3 for s in SHAPES]
    gs[4] = gs[4].contiguous(memory_format=torch.channels_last)
    return ps, gs


def _groups(params, over_b):
    return [{"params": [params[i] for i in GROUP_A]}, {"params": [params[i] for i in GROUP_B], **over_b}]


def _torch_run(cls, defaults, over_b, dtype, steps=3):
    """clip_grad_norm_(1.0) + the torch optimizer on the CPU in ``dtype``, gradients growing with the step."""
    ps, gs = _inputs()
    params = [p.clone().to(dtype).requires_grad_(True) for p in ps]
    opt = cls(_groups(params, over_b), **defaults)
    for step in range(steps):
        for i, (p, g) in enumerate(zip(params, gs)):
            p.grad = None if i == NO_GRAD else (g * (step + 1)).to(dtype)
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
    return [p.detach() for p in params]


def _fused_run(cls, defaults, over_b, steps=3, **kw):
    ps, gs = _inputs()
    params = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    opt = cls(_groups(params, over_b), **defaults, max_grad_norm=1.0, **kw)
    for step in range(steps):
        for i, (p, g) in enumerate(zip(params, gs)):
            p.grad = None if i == NO_GRAD else (g * (step + 1)).to(DEV)
        opt.step()
    return params, opt


def _check_parity(name, fused_cls, torch_cls, defaults, over_b):
    want = _torch_run(torch_cls, defaults, over_b, torch.float64)
    f32 = _torch_run(torch_cls, defaults, over_b, torch.float32)
    got, opt = _fused_run(fused_cls, defaults, over_b)
    ps, _ = _inputs()
    for i, (w, t, m) in enumerate(zip(want, f32, got)):
        own = (t.double() - w).abs().max().item()
        floor = 2 * float(np.spacing(np.float32(w.abs().max().item())))
        bound = max(4 * own, floor)
        err = (m.detach().cpu().double() - w).abs().max().item()
        print(f"{name} {tuple(SHAPES[i])}: fused-f64 {err:.3e}  torch f32-f64 {own:.3e}  bound {bound:.3e}")
        assert err <= bound, (name, SHAPES[i], err, bound)
        assert m.stride() == ps[i].stride()
    assert torch.equal(got[NO_GRAD].cpu(), ps[NO_GRAD]) and not opt.state.get(got[NO_GRAD])
    assert opt.table_builds >= 2              # (one table per group; fresh gradient tensors may or may not land on old addresses)
    return got, opt


def test_adamw_matches_torch():
    name, defaults, over_b = ADAMW
    got, opt = _check_parity(name, gnn.FusedAdamW, torch.optim.AdamW, defaults, over_b)
    st = opt.state[got[1]]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["step"] == 3


@pytest.mark.parametrize("case", SGD_CASES, ids=[c[0] for c in SGD_CASES])
def test_sgd_matches_torch(case):
    name, defaults, over_b = case
    got, opt = _check_parity("sgd-" + name, gnn.FusedSGD, torch.optim.SGD, defaults, over_b)
    for gi, group in enumerate(opt.param_groups):
        for p in group["params"]:
            if p is got[NO_GRAD]:
                continue
            want = {"step", "momentum_buffer"} if group["momentum"] != 0 else {"step"}
            assert set(opt.state[p]) == want and opt.state[p]["step"] == 3, (name, gi)


def test_adamw_without_weight_decay_is_adam_bit_for_bit():
    runs = []
    for cls in (gnn.FusedAdam, gnn.FusedAdamW):
        ps, gs = _inputs(3)
        params = [p.clone().to(DEV).requires_grad_(True) for p in ps[:5]]
        opt = cls(params, lr=1e-2, weight_decay=0.0)
        for step in range(3):
            for p, g in zip(params, gs):
                p.grad = (g * (step + 1)).to(DEV)
            opt.step()
        runs.append((params, opt))
    (pa, oa), (pw, ow) = runs
    for a, w in zip(pa, pw):
        assert torch.equal(a, w)
        assert torch.equal(oa.state[a]["exp_avg"], ow.state[w]["exp_avg"])
        assert torch.equal(oa.state[a]["exp_avg_sq"], ow.state[w]["exp_avg_sq"])
    assert not torch.equal(pa[1].cpu(), ps[1])


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_chunk_tables_are_reused_and_a_new_lr_takes_effect(kind):
    """Mirror of the second half of test_adam_and_clip: gradients rewritten IN PLACE -> no table rebuild; the learning rate a
    scheduler writes into the param group is a kernel argument and reaches the update."""
    fused_cls, torch_cls, kw = ((gnn.FusedAdamW, torch.optim.AdamW, dict(lr=1e-3)) if kind == "adamw" else
                                (gnn.FusedSGD, torch.optim.SGD, dict(lr=0.1, momentum=0.9)))
    ps, gs = _inputs(5)
    ps, gs = ps[2:5], gs[2:5]
    refs = {dt: [p.clone().to(dt).requires_grad_(True) for p in ps] for dt in (torch.float64, torch.float32)}
    o_ref = {dt: torch_cls(r, **kw) for dt, r in refs.items()}
    mine = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    o_mine = fused_cls(mine, **kw, max_grad_norm=1.0)
    for p in mine:
        p.grad = torch.zeros_like(p)
    before = None
    for step in range(6):
        if step == 3:
            builds = o_mine.table_builds
            before = [m.detach().clone() for m in mine]
        if step >= 3:
            for o in (*o_ref.values(), o_mine):
                o.param_groups[0]["lr"] = kw["lr"] * (step - 1)
        for dt, r in refs.items():
            for p, g in zip(r, gs):
                p.grad = (g * 0.1 * (step + 1)).to(dt)
            torch.nn.utils.clip_grad_norm_(r, 1.0)
            o_ref[dt].step()
        for m, g in zip(mine, gs):
            m.grad.copy_((g * 0.1 * (step + 1)).to(DEV))
        o_mine.step()
    assert builds == 1 and o_mine.table_builds == 1
    for w, t, m, b in zip(refs[torch.float64], refs[torch.float32], mine, before):
        own = (t.detach().double() - w.detach()).abs().max().item()
        bound = max(4 * own, 2 * float(np.spacing(np.float32(w.abs().max().item()))))
        err = (m.detach().cpu().double() - w.detach()).abs().max().item()
        print(f"{kind} reuse {tuple(m.shape)}: fused-f64 {err:.3e}  torch f32-f64 {own:.3e}  bound {bound:.3e}")
        assert err <= bound, (kind, err, bound)
        assert (m.detach() - b).abs().max().item() > 10 * bound       # the later steps (new lr) moved the parameters


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_update_rewrites_the_bf16_gemm_operands(kind, monkeypatch):
    """Pattern of test_adam_rewrites_the_bf16_gemm_operands: the operand objects stay, hold a fresh cast's bits, no cast launch."""
    lin = torch.randn(96, 200, device=DEV).requires_grad_(True)
    cl = torch.randn(64, 32, 3, 3, device=DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    params = [lin, cl]
    opt = gnn.FusedAdamW(params, lr=1e-2) if kind == "adamw" else gnn.FusedSGD(params, lr=0.1, momentum=0.9, weight_decay=1e-2)
    first = [gnn.gemm_weight(p, torch.bfloat16) for p in params]
    casts = []
    real_cast = ops.cast
    monkeypatch.setattr(ops, "cast", lambda *a, **k: (casts.append(1), real_cast(*a, **k))[1])
    for p in params:
        p.grad = torch.zeros_like(p)
    for _ in range(3):
        old = [p.detach().clone() for p in params]
        for p in params:
            p.grad.copy_(torch.randn_like(p))
        opt.step()
        casts.clear()
        now = [gnn.gemm_weight(p, torch.bfloat16) for p in params]
        assert not casts
        assert now[0] is first[0] and now[1] is first[1]
        assert not torch.equal(lin, old[0]) and not torch.equal(cl, old[1])
        assert torch.equal(now[0], lin.detach().to(torch.bfloat16))
        assert torch.equal(now[1], cl.detach().permute(0, 2, 3, 1).reshape(64, -1).to(torch.bfloat16))
    assert opt.table_builds == 1


@pytest.mark.parametrize("kind", ["adamw", "sgd", "sgd-dampening"])
def test_capturable_eager_steps_equal_the_host_form_bit_for_bit(kind):
    """Hyper-parameters and step count from device memory (capturable) against kernel arguments; the learning rate changes
    between the steps like a scheduler's write (sync_lr)."""
    if kind == "adamw":
        make = partial(gnn.FusedAdamW, lr=1e-2, weight_decay=1e-2)
    else:
        make = partial(gnn.FusedSGD, lr=0.1, momentum=0.9, weight_decay=1e-2, dampening=0.5 if kind == "sgd-dampening" else 0.0)
    runs = []
    for capturable in (False, True):
        ps, gs = _inputs(7)
        params = [p.clone().to(DEV).requires_grad_(True) for p in ps[:5]]
        opt = make([{"params": params[:3]}, {"params": params[3:], "lr": 0.02}], capturable=capturable)
        for step in range(3):
            for group in opt.param_groups:
                group["lr"] = group["lr"] * 0.7
            for p, g in zip(params, gs):
                p.grad = (g * (step + 1)).to(DEV)
            opt.step()
        runs.append((params, opt))
    (ph, oh), (pc, oc) = runs
    for h, c in zip(ph, pc):
        assert torch.equal(h, c)
        for k, v in oh.state[h].items():
            assert torch.equal(v, oc.state[c][k]) if isinstance(v, torch.Tensor) else v == oc.state[c][k]
    assert float(oc.device_state(0)[0]) == 3.0
    assert abs(float(oc.device_state(1)[1]) - 0.02 * 0.7 ** 3) < 1e-9


GRAPH_CASES = [("adamw", "f32"), ("adamw", "bf16"), ("sgd", "f32"), ("sgd", "bf16")]


@pytest.mark.parametrize("kind,precision", GRAPH_CASES, ids=[f"{k}-{p}" for k, p in GRAPH_CASES])
def test_captured_step_equals_the_eager_twin(kind, precision):
    """GraphedTrainStep with FusedAdamW(capturable=True) / FusedSGD(momentum=0.9, capturable=True) on the tiny DOFA task (frozen
    encoder, batch 2, 3x112x112): four replays with one eager step in between against an all-eager twin; every loss bit for bit,
    no derived operand out of date.  One process per scenario (see test_hip_tasks.py on captures sharing a process)."""
    worker = Path(__file__).with_name("_optimizer_graph_worker.py")
    env = dict(os.environ, MASTER_PORT=str(29900 + os.getpid() % 1000))
    run = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(worker), kind, precision], capture_output=True, text=True, env=env)
    if run.returncode in (124, 134, 137, 139) or run.returncode < 0:
        pytest.exit(f"the captured-step worker ({kind}, {precision}) ended with status {run.returncode}: nothing further is started on "
                    f"the GPU\n{run.stdout[-2000:]}{run.stderr[-4000:]}", returncode=1)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    print(res)
    assert res["replays"] == 4 and res["eager_steps_in_between"] == 1, res
    assert res["losses_graphed"] == res["losses_eager"], res
    assert len(set(res["losses_eager"])) == 5, res                     # the task trains: no two steps give the same loss
    assert res["derived_operands_wrong"] == 0, res
    assert res["device_step"] == 7.0 and res["eager_twin_step"] == 7, res     # two warm-up steps of the capture + five
    if precision == "bf16":
        assert res["operands_under_the_optimizers_care"] >= 8 and res["derived_operands_checked"] >= 8, res


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_minitrainer_fuses_captures_and_resumes(kind, tmp_path):
    """MiniTrainer.fit with torch.optim.AdamW / SGD from configure_optimizers: the fused class runs the step, the step is captured,
    and a checkpoint reloaded into a fresh task + trainer continues with the same bits after one more step."""
    import test_hip_tasks as T
    from gdlhip.trainer import MiniTrainer, seed_everything
    torch_opt = partial(torch.optim.AdamW, lr=1e-3) if kind == "adamw" else partial(torch.optim.SGD, lr=0.01, momentum=0.9)
    fused_cls = gnn.FusedAdamW if kind == "adamw" else gnn.FusedSGD
    batches = [T.synthetic_batch(2, 3, 112, 5, s) for s in (1, 2, 3)]
    for bt in batches:
        bt["mask"] = (bt["image"][:, :1] * 1.2 + 2).clamp(0, 4).long()

    def make():
        _, task = T._dofa_task(optimizer=torch_opt, scheduler=partial(torch.optim.lr_scheduler.StepLR, step_size=2, gamma=0.5),
                               scheduler_config={"interval": "step", "frequency": 1})
        for blk in task.model.encoder.blocks:
            blk.drop_prob = 0.0
        task.model.aux_head.dropout_ratio = 0.0
        return task

    seed_everything(42)
    task = make()
    tr = MiniTrainer(max_epochs=2, precision="bf16-mixed", default_root_dir=str(tmp_path), graph_step=True)
    tr.fit(task, train_dataloaders=batches, val_dataloaders=None)
    opt = tr._optimizers[0]
    assert type(opt) is fused_cls and opt.capturable
    assert tr.global_step == 6 and tr.graphed_steps == 6, (tr.graphed_steps, getattr(tr, "capture_traceback", ""))
    lr0 = 1e-3 if kind == "adamw" else 0.01
    assert opt.param_groups[0]["lr"] == lr0 * 0.5 ** 3 and abs(float(opt.device_state(0)[1]) - lr0 * 0.25) < 1e-9   # (last sync: step 6)
    some = next(p for p in task.parameters() if p.requires_grad)
    assert opt.state[some]["step"] == 6
    path = tmp_path / "resume.ckpt"
    tr.save_checkpoint(task, path)
    saved = torch.load(path)["optimizer_states"][0]
    keys = {k for st in saved["state"].values() for k in st}
    assert keys == ({"step", "exp_avg", "exp_avg_sq"} if kind == "adamw" else {"step", "momentum_buffer"})

    fresh = make()
    tr2 = MiniTrainer(max_epochs=1, precision="bf16-mixed", default_root_dir=str(tmp_path / "b"))
    tr2.load_checkpoint(fresh, path)
    fresh.trainer = tr2
    tr.training = tr2.training = True
    opt2 = tr2._maybe_fuse(fresh.configure_optimizers()[0][0], torch.device(DEV))
    assert type(opt2) is fused_cls and not opt2.capturable
    opt2.load_state_dict(saved)

    batch = T._to_dev(batches[0])
    losses = []
    for t, o in ((task, opt), (fresh, opt2)):
        t.train()
        o.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = t.training_step(batch, 0)
        loss.backward()
        o.step()
        losses.append(loss.item())
    assert losses[0] == losses[1], losses
    mine, theirs = dict(task.named_parameters()), dict(fresh.named_parameters())
    moved = 0
    for n, p in mine.items():
        assert torch.equal(p, theirs[n]), n
    ckpt_sd = torch.load(path)["state_dict"]
    for n, p in task.model.named_parameters():
        if p.requires_grad:
            moved += int(not torch.equal(p.detach().cpu(), ckpt_sd["model." + n]))
    assert moved > 0 and opt2.state[next(p for p in fresh.parameters() if p.requires_grad)]["step"] == 7
