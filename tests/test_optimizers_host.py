"""gdlhip.nn.FusedAdamW / FusedSGD, the parts that need no GPU: constructor contract, state-dict keys after loading a state
written by torch.optim.AdamW / SGD, and the cases in which MiniTrainer leaves the optimizer as torch's own."""

import pytest
import torch

gdlhip = pytest.importorskip("gdlhip")
from gdlhip import nn as gnn  # noqa: E402
from gdlhip.trainer import MiniTrainer  # noqa: E402


def _params():
    return [torch.randn(5, 3, requires_grad=True), torch.randn(7, requires_grad=True)]


def test_constructor_defaults_follow_torch():
    ps = _params()
    w = gnn.FusedAdamW(ps)
    assert w.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    assert w.max_grad_norm is None and w.capturable is False and w.table_builds == 0 and w.CHUNK == 65536
    s = gnn.FusedSGD(ps, lr=0.1)
    assert s.defaults == dict(lr=0.1, momentum=0, dampening=0, weight_decay=0, nesterov=False)
    a = gnn.FusedAdam(ps)
    assert a.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0) and a.CHUNK == 65536
    for opt in (w, s, a):
        for name in ("step", "refresh_derived", "device_state", "sync_lr", "note_replay"):
            assert callable(getattr(opt, name))
    with pytest.raises(TypeError):
        gnn.FusedSGD(ps)                                  # lr is required, as in torch.optim.SGD's documented signature


def test_sgd_constructor_validation():
    ps = _params()
    for kw in (dict(lr=-0.1), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1e-2),
               dict(lr=0.1, nesterov=True), dict(lr=0.1, nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError):
            gnn.FusedSGD(ps, **kw)
        with pytest.raises(ValueError):                   # the same arguments are errors in torch
            torch.optim.SGD(ps, **kw)
    gnn.FusedSGD(ps, lr=0.1, nesterov=True, momentum=0.9)


def _stepped(cls, **kw):
    ps = _params()
    opt = cls(ps, **kw)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    opt.step()
    return opt.state_dict()


def test_state_written_by_torch_loads_under_torch_key_names():
    ps = _params()
    w = gnn.FusedAdamW(ps)
    w.load_state_dict(_stepped(torch.optim.AdamW, lr=1e-3))
    for p in ps:
        assert set(w.state[p]) == {"step", "exp_avg", "exp_avg_sq"}
        assert w.state[p]["step"] == 2 and isinstance(w.state[p]["step"], int)
        assert w.state[p]["exp_avg"].shape == p.shape
    assert set(w.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    s = gnn.FusedSGD(ps, lr=0.1, momentum=0.9)
    s.load_state_dict(_stepped(torch.optim.SGD, lr=0.1, momentum=0.9))
    for p in ps:
        assert set(s.state[p]) == {"momentum_buffer"} and s.state[p]["momentum_buffer"].shape == p.shape
    assert s.param_groups[0]["momentum"] == 0.9
    plain = gnn.FusedSGD(ps, lr=0.1)
    plain.load_state_dict(_stepped(torch.optim.SGD, lr=0.1))
    assert all("momentum_buffer" not in plain.state.get(p, {}) for p in ps)
    # the first fused step after such a load is not a "first step" (torch: the buffer exists, so it is not re-cloned)
    for p in ps:
        s._init_state(s.param_groups[0], p, s.state[p])
        assert set(s.state[p]) == {"momentum_buffer", "step"} and s.state[p]["step"] + 1 > 1
        plain._init_state(plain.param_groups[0], p, plain.state[p])
        assert set(plain.state[p]) == {"step"} and plain.state[p]["step"] == 0


def test_maybe_fuse_leaves_the_optimizer_alone_when_it_must():
    ps = _params()
    tr = MiniTrainer(gradient_clip_val=1.0)
    cpu = torch.device("cpu")
    for opt in (torch.optim.Adam(ps), torch.optim.AdamW(ps), torch.optim.SGD(ps, lr=0.1)):
        assert tr._maybe_fuse(opt, cpu) is opt
    cuda = torch.device("cuda", 0)                         # (nothing touches the device before the optimizer's first step)
    for opt in (torch.optim.AdamW(ps, amsgrad=True), torch.optim.AdamW(ps, maximize=True), torch.optim.SGD(ps, lr=0.1, maximize=True),
                torch.optim.Adam(ps, amsgrad=True), torch.optim.RMSprop(ps)):
        assert tr._maybe_fuse(opt, cuda) is opt

    class MySGD(torch.optim.SGD):
        pass

    opt = MySGD(ps, lr=0.1)
    assert tr._maybe_fuse(opt, cuda) is opt                # exact types only
    for opt, cls in ((torch.optim.AdamW(ps, lr=2e-3, weight_decay=0.05), gnn.FusedAdamW),
                     (torch.optim.SGD(ps, lr=0.1, momentum=0.9, nesterov=True), gnn.FusedSGD), (torch.optim.Adam(ps), gnn.FusedAdam)):
        fused = tr._maybe_fuse(opt, cuda, capturable=True)
        assert type(fused) is cls and fused.capturable and fused.max_grad_norm == 1.0
        assert fused.param_groups is opt.param_groups      # schedulers keep writing lr into the same dicts
    opt = torch.optim.AdamW(ps)
    assert MiniTrainer(use_fused_adam=False)._maybe_fuse(opt, cuda) is opt
