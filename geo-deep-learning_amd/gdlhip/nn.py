"""Autograd-aware fused ops + precision policy + packed-weight cache.

Everything here is host logic around libgdlhip.so: forward AND backward arithmetic run in the
HIP kernels (``gdlhip.ops``); ``torch.autograd.Function`` only records the graph so that the
reference's ``loss.backward()`` / DDP hooks keep working unchanged.
"""

from __future__ import annotations

import contextlib
import math
import os

import logging
import weakref
from typing import NamedTuple

import torch
import torch.distributed as dist
from torch import Tensor, nn
from torch.autograd import Function

from . import ops
from .ops import ACT_GELU, ACT_NONE, ACT_RELU, ACT_RESID_RELU  # noqa: F401


_log = logging.getLogger(__name__)
_WARNED_FP16 = False
_WARNED_FALLBACK: set = set()


def warn_unfused(what: str, why: str) -> None:
    """One log line per (path, reason) when a grid-limit / shape guard sends a fused node down its unfused path."""
    if (what, why) not in _WARNED_FALLBACK:
        _WARNED_FALLBACK.add((what, why))
        _log.warning("gdlhip: %s runs UNFUSED (%s): correct, but several times slower", what, why)


# ------------------------------------------------------------------ precision policy
# A/B switch (tools): GDL_LAUNCH_FUSION=0 restores one launch per DropPath draw / BatchNorm counter / parameter cast
LAUNCH_FUSION = os.environ.get("GDL_LAUNCH_FUSION", "1") != "0"
_COUNTER_BATCH: list | None = None


@contextlib.contextmanager
def counter_batch():
    """Inside this context the ``num_batches_tracked += 1`` of every train-mode BatchNorm (nn.BatchNorm2d.forward) is collected
    and applied by ONE multi-tensor launch at exit instead of one launch per layer (21 in DOFA + UperNet, 62 in UNet++); the
    model forwards wrap themselves in it.  Outside of it ``bump`` increments at once."""
    global _COUNTER_BATCH
    if _COUNTER_BATCH is not None or not LAUNCH_FUSION:      # nested: the outermost context applies
        yield
        return
    _COUNTER_BATCH = []
    try:
        yield
    finally:
        pending, _COUNTER_BATCH = _COUNTER_BATCH, None
        if pending:
            torch._foreach_add_(pending, 1)


def bump(counter: Tensor | None) -> None:
    if counter is None:
        return
    if _COUNTER_BATCH is None:
        counter.add_(1)
    else:
        _COUNTER_BATCH.append(counter)


_KEEP_CACHE: dict = {}


def drop_path_scales(probs: list[float], batch: int, device) -> list[tuple[Tensor | None, Tensor | None]]:
    """The per-sample DropPath scales (mask / keep, timm ``drop_path`` with scale_by_keep) of a whole encoder pass, two draws per
    block (attention branch, MLP branch), from ONE Bernoulli launch and ONE division instead of two launches per draw (46 per
    DOFA-base step; at the reference's batch of 4 these sub-5-us launches are 2 % of the step).  ``probs[i]`` = block i's drop
    probability; blocks with probability 0 get (None, None).  Rows of one [2 n, B] tensor, dense."""
    live = [i for i, p_ in enumerate(probs) if p_ > 0.0]
    out: list[tuple[Tensor | None, Tensor | None]] = [(None, None)] * len(probs)
    if not live:
        return out
    if not LAUNCH_FUSION:
        for i in live:
            out[i] = tuple((torch.empty(batch, device=device, dtype=torch.float32).bernoulli_(1.0 - probs[i]) / (1.0 - probs[i]))
                           for _ in (0, 1))
        return out
    key = (str(device), tuple(probs[i] for i in live))
    keep = _KEEP_CACHE.get(key)
    if keep is None:
        keep = torch.tensor([1.0 - probs[i] for i in live for _ in (0, 1)], dtype=torch.float32, device=device).view(-1, 1)
        _KEEP_CACHE[key] = keep
    scales = torch.bernoulli(keep.expand(-1, batch)) / keep
    for j, i in enumerate(live):
        out[i] = (scales[2 * j], scales[2 * j + 1])
    return out


def compute_dtype() -> torch.dtype:
    """bf16 MFMA path under ``torch.autocast('cuda', bfloat16/float16)``, exact-f32 MFMA otherwise.

    The reference selects precision through Lightning's ``precision:`` flag, i.e. autocast
    (configs/dofa_config_RGB.yaml:12); the kernels accumulate in f32 either way.
    """
    if torch.is_autocast_enabled("cuda"):
        global _WARNED_FP16
        if not _WARNED_FP16 and torch.get_autocast_dtype("cuda") == torch.float16:
            # the reference's `precision: 16-mixed` (configs/dofa_config_RGB.yaml:12): there is no fp16 kernel set here
            _log.warning("gdlhip: fp16 autocast is computed in bf16 (f32 accumulation) by the HIP kernels; no loss scaling is "
                         "needed or applied")
            _WARNED_FP16 = True
        return torch.bfloat16
    return torch.float32


# ------------------------------------------------------------------ packed-weight cache
_RAW_WRITES: dict = {}   # id(param) -> number of raw-pointer updates (tensor._version does not see them)
_CACHE: dict = {}
_CACHE_BUILDS = [0]      # how often an operand was (re)built: whoever keeps lists of cache entries (FusedAdam.refresh_derived) rescans on a change


def mark_updated(p: Tensor) -> None:
    """Called for every tensor a kernel rewrites through a raw pointer (fused optimizer: parameters; single-GPU
    BatchNorm statistics kernel: running_mean / running_var) -- ``tensor._version`` does not see those writes."""
    if id(p) not in _RAW_WRITES:
        weakref.finalize(p, _RAW_WRITES.pop, id(p), None)
    _RAW_WRITES[id(p)] = _RAW_WRITES.get(id(p), 0) + 1


def _mark_running(running_mean: Tensor | None, running_var: Tensor | None) -> None:
    """The running estimates were written through raw pointers: invalidate the eval-mode fold cache."""
    if running_mean is not None:
        mark_updated(running_mean)
        mark_updated(running_var)


def cached(params: tuple, kind: str, builder):
    """Memoise ``builder()`` on the identity + version of ``params`` (tensors).  Frozen
    parameters never change version, so e.g. the DOFA dynamic patch-embed kernel of a frozen
    encoder is generated once per sensor, not once per step.  An entry dies with the tensors it was
    built from (weakref finalizers), so the cache never pins the device tensors of a dead model."""
    key = (kind, *[id(p) for p in params])
    ver = tuple((p._version, _RAW_WRITES.get(id(p), 0), p.data_ptr()) for p in params)
    hit = _CACHE.get(key)
    # ids (and allocator addresses) are recycled once a model is garbage collected: an entry only counts when it
    # was built from these very tensor objects
    if hit is not None and hit[0] == ver and all(r() is p for r, p in zip(hit[2], params)):
        return hit[1]
    val = builder()
    _CACHE_BUILDS[0] += 1
    if hit is None:
        for p in params:
            weakref.finalize(p, _CACHE.pop, key, None)
    _CACHE[key] = (ver, val, tuple(weakref.ref(p) for p in params))
    return val


def conv_weight_matrix(weight: Tensor) -> Tensor:
    """[N,C,R,S] conv parameter -> f32 [N, R*S*C] view (free when stored channels_last)."""
    n = weight.shape[0]
    w = weight.detach().permute(0, 2, 3, 1)
    if not w.is_contiguous():
        w = w.contiguous()  # parameter not stored channels_last: one repack (cached by caller)
    return w.reshape(n, -1)


def gemm_weight(weight: Tensor, cd: torch.dtype) -> Tensor:
    """GEMM operand ([N, K] K-contiguous, compute dtype) of a Linear / conv parameter."""
    def build():
        w = weight.detach() if weight.dim() == 2 else conv_weight_matrix(weight)
        w = w if w.is_contiguous() else w.contiguous()
        return w if cd == torch.float32 else ops.cast(w, cd)
    return cached((weight,), f"gemm:{cd}", build)


def gemm_weight_shadow(weight: Tensor):
    """(cache key, bf16 tensor) of ``gemm_weight(weight, bf16)`` when that operand exists and is a plain cast of the parameter's
    dense storage (same element order) -- then the fused optimizer rewrites it together with the parameter
    (gdl_multi_adam's `shadow` column) and ``refresh_shadow`` revalidates the cache entry; None otherwise."""
    key = (f"gemm:{torch.bfloat16}", id(weight))
    hit = _CACHE.get(key)
    if hit is None or hit[2][0]() is not weight:
        return None
    val = hit[1]
    if val.dtype != torch.bfloat16 or val.numel() != weight.numel() or not val.is_contiguous() or weight.dtype != torch.float32:
        return None
    if weight.dim() == 2:
        same_order = weight.is_contiguous()
    else:
        same_order = weight.dim() == 4 and weight.permute(0, 2, 3, 1).is_contiguous()
    return (key, val) if same_order else None


def refresh_shadow(key, val: Tensor, weight: Tensor) -> None:
    """After the optimizer rewrote ``weight`` AND its bf16 shadow ``val``: the cache entry is current again."""
    hit = _CACHE.get(key)
    if hit is not None and hit[1] is val and hit[2][0]() is weight:
        _CACHE[key] = ((((weight._version, _RAW_WRITES.get(id(weight), 0), weight.data_ptr())),), val, hit[2])


# bf16 operands DERIVED from a conv parameter in another element order (channel slice, tap-major, data gradient): the fused
# optimizer rebuilds all of them in ONE launch behind its update (gdl_multi_repack) and revalidates their cache entries, like the
# plain bf16 copies above -- id(weight) -> {cache key: (mode, c0, c1)}
_DERIVED: dict = {}
REPACK_SLICE, REPACK_TAPS, REPACK_DGRAD = 0, 1, 2
REPACK_FUSION = os.environ.get("GDL_REPACK_FUSION", "1") != "0"   # A/B switch: 0 = derived operands are rebuilt on their next use


def _register_derived(weight: Tensor, kind: str, cd: torch.dtype, mode: int, c0: int, c1: int) -> None:
    if cd != torch.bfloat16 or not LAUNCH_FUSION or not REPACK_FUSION or weight.dtype != torch.float32 or not weight.requires_grad:
        return
    if not (weight.dim() == 4 and weight.permute(0, 2, 3, 1).is_contiguous()):
        return                                            # (the kernel reads the parameter's dense [N][T][C] storage)
    ent = _DERIVED.get(id(weight))
    if ent is None:
        ent = _DERIVED[id(weight)] = {}
        weakref.finalize(weight, _DERIVED.pop, id(weight), None)
    ent[(kind, id(weight))] = (mode, c0, c1)


def derived_operands(weight: Tensor) -> list:
    """[(cache key, bf16 tensor, mode, c0, c1)] of the derived operands of ``weight`` that exist in the cache right now."""
    out = []
    for key, (mode, c0, c1) in _DERIVED.get(id(weight), {}).items():
        hit = _CACHE.get(key)
        if hit is None or hit[2][0]() is not weight:
            continue
        val = hit[1]
        if isinstance(val, Tensor) and val.dtype == torch.bfloat16 and val.is_contiguous():
            out.append((key, val, mode, c0, c1))
    return out


def adopt_operand(key, val: Tensor, weight: Tensor) -> None:
    """``val`` was just rewritten from the CURRENT ``weight`` by a kernel that holds its address (a hipGraph replay of the
    optimizer's update): make it THE cache entry of ``key`` again, whatever an eager step put there in between.  Without this
    an eager step between two replays builds new operand tensors, the eager update rewrites those, and the next replay's forward
    reads operands that miss one update."""
    hit = _CACHE.get(key)
    if hit is None or hit[1] is not val:
        _CACHE_BUILDS[0] += 1
    if hit is not None and hit[2][0]() is weight:
        refs = hit[2]
    else:
        refs = (weakref.ref(weight),)
        if hit is None:
            weakref.finalize(weight, _CACHE.pop, key, None)
    _CACHE[key] = (((weight._version, _RAW_WRITES.get(id(weight), 0), weight.data_ptr()),), val, refs)


def dgrad_weight(weight: Tensor, cd: torch.dtype) -> Tensor:
    """Flipped / transposed operand for the data gradient of a conv parameter."""
    def build():
        n, c, r, s = weight.shape
        return ops.pack_dgrad(conv_weight_matrix(weight), n, r * s, c, cd)
    _register_derived(weight, f"dgrad:{cd}", cd, REPACK_DGRAD, 0, weight.shape[1])
    return cached((weight,), f"dgrad:{cd}", build)


class _ToCompute(Function):
    @staticmethod
    def forward(ctx, x, cd):
        ctx.in_dtype = x.dtype
        return ops.copy_cast(x, out_dtype=cd)

    @staticmethod
    def backward(ctx, g):
        return ops.copy_cast(g, out_dtype=ctx.in_dtype), None


def to_compute(x: Tensor, cd: torch.dtype) -> Tensor:
    """NHWC tensor in the compute dtype (strided copy+cast through the identity resize)."""
    if x.dtype == cd:
        return x
    if x.requires_grad and torch.is_grad_enabled():
        return _ToCompute.apply(x, cd)
    return ops.copy_cast(x, out_dtype=cd)


def _world(group=None) -> int:
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def _sync_world(sync_group) -> int:
    """Ranks a train-mode BatchNorm merges its statistics over; ``sync_group``: False = none (nn.BatchNorm2d), None = default group."""
    return _world(sync_group) if sync_group is not False else 1


def _bn_sync_momentum(norm: nn.Module) -> tuple:
    """(sync_group, momentum) of a BatchNorm module, as the training nodes take them."""
    return (norm.process_group if isinstance(norm, nn.SyncBatchNorm) else False), (0.1 if norm.momentum is None else norm.momentum)


_EVAL_BN_GRAD_MSG = ("gdlhip: autograd through eval-mode BatchNorm is not implemented; call under "
                     "torch.no_grad() for inference or model.train() for training")


# ------------------------------------------------------------------ SyncBatchNorm exchange
FUSE_SYNC_MESSAGE = os.environ.get("GDL_SYNC_MESSAGE_KERNELS", "1") != "0"   # A/B switch: 0 = the message is built by torch expressions
# 1 = every statistics exchange first checks that its pivot (running_mean) is the same on all ranks: two more all-reduces per message
SYNC_CHECK_PIVOT = os.environ.get("GDL_SYNC_CHECK_PIVOT", "0") == "1"


def check_sync_pivot(pivot: Tensor | None, group=None) -> None:
    """The pivoted message is only right if every rank subtracts the SAME pivot (SyncBatchNorm without DDP, or with
    broadcast_buffers=False after divergent loads, breaks that silently).  With GDL_SYNC_CHECK_PIVOT=1: raise if not."""
    if not SYNC_CHECK_PIVOT or pivot is None:
        return
    lo, hi = pivot.clone(), pivot.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
    if not torch.equal(lo, hi):
        raise RuntimeError("gdlhip: running_mean differs between the ranks: the SyncBatchNorm statistics message needs identical "
                           "buffers on every rank (DDP with broadcast_buffers=True, or load the same state everywhere)")


def sync_message(mean: Tensor, var: Tensor, n: float, pivot: Tensor | None = None) -> list[Tensor]:
    """One rank's share of the statistics message as torch expressions (what ops.syncbn_pack writes): the sums are taken about
    ``pivot``, per-channel values that every rank holds identically (the layer's running_mean; None = 0), so that the f32
    message cancels digits in proportion to ((global mean - pivot) / std)^2 and not to (mean / std)^2."""
    d = mean if pivot is None else mean - pivot
    return [d * n, (var + d * d) * n, mean.new_full((1,), n)]


def sync_message_stats(packed: Tensor, c: int, pivot: Tensor | None = None):
    """(global mean, global biased variance, global count) out of the summed message of sync_message (ops.syncbn_unpack)."""
    total = packed[2 * c]
    d = packed[:c] / total
    gvar = (packed[c:2 * c] / total - d * d).clamp_min_(0).contiguous()
    gmean = (d if pivot is None else d + pivot).contiguous()
    return gmean, gvar, total


def _sync_pivot(running_mean: Tensor | None, c: int) -> Tensor | None:
    """The message pivot of a layer with c (possibly padded) channels: its running_mean (identical on every rank under DDP, which
    broadcasts the buffers, and under SyncBatchNorm, which updates them alike), zero-padded; None (pivot 0) without buffers."""
    if running_mean is None:
        return None
    rm = running_mean.detach()
    return (rm if rm.numel() == c else nn.functional.pad(rm, (0, c - rm.numel()))).contiguous()


def sync_batch_stats(mean: Tensor, var: Tensor, group=None, count: int | None = None, pivot: Tensor | None = None):
    """Merge per-rank batch statistics into global ones (nn.SyncBatchNorm forward): count-weighted, so a
    ragged last batch (ranks with different pixel counts) merges exactly like torch's all_gather of
    [mean, invstd, count] does -- in ONE small all-reduce of 2C + 1 floats: sum_r n_r * [mean_r - r, E_r[(x - r)^2], 1]
    about the pivot r = ``pivot`` (see sync_message; it must be identical on every rank).
    Returns (global mean, global biased variance, global count); the count stays a 0-dim DEVICE tensor (no host
    read-back: 21 layers per step would mean 21 stream syncs)."""
    n = float(count if count is not None else 1)
    c = mean.numel()
    check_sync_pivot(pivot, group)
    if mean.is_cuda and FUSE_SYNC_MESSAGE:
        # one pack kernel, the all-reduce, one unpack kernel (the torch expressions below are ~12 one-line launches per layer)
        packed = torch.empty(2 * c + 1, device=mean.device, dtype=torch.float32)
        ops.syncbn_pack(mean, var, n, packed, pivot)
        dist.all_reduce(packed, group=group)
        SYNC_MESSAGES[0] += 1
        gmean, gvar = ops.syncbn_unpack(packed, c, pivot=pivot)
        return gmean, gvar, packed[2 * c]
    packed = torch.cat(sync_message(mean, var, n, pivot))
    dist.all_reduce(packed, group=group)
    SYNC_MESSAGES[0] += 1
    return sync_message_stats(packed, c, pivot)


def update_running_stats(running_mean, running_var, mean, var, momentum: float, count) -> None:
    """nn.BatchNorm2d running-stat update with the UNBIASED variance; ``count`` int or 0-dim tensor."""
    running_mean.mul_(1 - momentum).add_(mean, alpha=momentum)
    if isinstance(count, Tensor):
        running_var.mul_(1 - momentum).add_(var * (momentum * count / (count - 1).clamp_min(1)))
    else:
        running_var.mul_(1 - momentum).add_(var, alpha=momentum * count / max(count - 1, 1))


def sync_sum_pair(a: Tensor, b: Tensor, group=None) -> tuple[Tensor, Tensor]:
    """all-reduce(SUM) of the two BN-backward reductions in one message (SyncBatchNorm backward)."""
    packed = torch.stack([a, b])
    dist.all_reduce(packed, group=group)
    SYNC_MESSAGES[1] += 1
    return packed[0].contiguous(), packed[1].contiguous()


# ------------------------------------------------------------------ train-mode BatchNorm protocol of the conv + BN nodes
# forward:  local statistics -> count-weighted cross-rank merge -> running-estimate update -> invalidate the eval-mode fold cache
# backward: sums pass -> ONE all-reduce of the pair -> rescale to the global count -> dx pass
def _bn_local_stats(y, stats_done, running_mean=None, running_var=None, momentum: float = 0.1):
    """This rank's (mean, biased var): ``stats_done`` when they came with y (_cba_conv), else one pass that also updates the
    running buffers it is given."""
    return stats_done if stats_done is not None else ops.bn_stats(y, running_mean, running_var, momentum)


def _bn_train_stats(y, n, running_mean, running_var, momentum, sync_group, stats_done=None):
    """Forward half for the conv output y (n real channels of y.shape[-1]: gdlhip.cnn pads) -> (mean, var, world, p_local,
    p_share, total); p_share = p_local / total and total (global pixel count, 0-dim DEVICE tensor) are None in one process.
    A kernel writes the running buffers only for one process and unpadded channels -- the pass here or the producer of
    ``stats_done`` (_cba_conv gave it the buffers on the same condition); else update_running_stats on the real channels."""
    world = _sync_world(sync_group)
    p_local, p_share, total = y.numel() // y.shape[-1], None, None
    in_kernel = world == 1 and y.shape[-1] == n
    mean, var = _bn_local_stats(y, stats_done, *((running_mean, running_var) if in_kernel else (None, None)), momentum)
    if world > 1:
        mean, var, total = sync_batch_stats(mean, var, sync_group or None, count=p_local, pivot=_sync_pivot(running_mean, mean.numel()))
    if in_kernel:
        _mark_running(running_mean, running_var)
    elif running_mean is not None:
        update_running_stats(running_mean, running_var, mean[:n], var[:n], momentum, p_local if total is None else total)
    if world > 1:
        p_share = p_local / total          # this rank's share of the global pixel count (device scalar)
    return mean, var, world, p_local, p_share, total


def _bn_sync_sums(dgamma, dbeta, sync_group, world, p_share=None):
    """The two backward sums as a dx kernel takes them: all-reduced in one message and, given ``p_share``, scaled by p_local /
    P_global so that the kernel's division by the LOCAL count gives the global mean (a kernel that reads the global count passes none)."""
    if world == 1:
        return dgamma, dbeta
    sg, sb = sync_sum_pair(dgamma, dbeta, sync_group or None)
    return (sg, sb) if p_share is None else (sg * p_share, sb * p_share)


def _bn_train_backward(y, gout, mean, var, g, b, eps, relu, sync_group, world, p_local, p_share):
    """(dy written over y, dgamma, dbeta) of BatchNorm(batch stats) (+ ReLU): sums pass, exchange, dx pass."""
    if gout.dtype != y.dtype:
        gout = to_compute(gout, y.dtype)
    dgamma, dbeta = ops.bn_bwd_reduce(y, gout, mean, var, g, b, eps, relu)
    sg, sb = _bn_sync_sums(dgamma, dbeta, sync_group, world, p_share)
    dy = ops.bn_bwd_dx(y, gout, mean, var, g, b, eps, relu, sg, sb, p_local, out=y)
    return dy, dgamma, dbeta


FUSE_UP4 = True   # A/B switch: False = materialise the x4 upsample and run the ordinary 3x3 kernel
FUSE_TAPSUM = True   # A/B switch: False = round-2 forward of resized-input convolutions (sub-pixel phases / concat buffer)
FUSE_TAPSUM_STATS = True   # A/B switch: False = separate BatchNorm statistics pass over the gather-sum's output


def tap_weight(weight: Tensor, cd: torch.dtype, c0: int = 0, c1: int | None = None) -> Tensor:
    """[9 N, C'] operand of the low-resolution forward of conv3x3(resize(x)) (ops.resize_conv3x3_fwd_sum): row t * N + n
    is filter tap t = 3 r + s of output channel n over the input-channel slice c0:c1 -- the nine tap products
    z = [W_0 x, ..., W_8 x] are then ONE 1x1 convolution with 9 N output channels."""
    def build():
        n, c = weight.shape[0], weight.shape[1]
        w = conv_weight_matrix(weight).view(n, 9, c)[:, :, c0:c1].permute(1, 0, 2).reshape(9 * n, -1).contiguous()
        return w if cd == torch.float32 else ops.cast(w, cd)
    if tuple(weight.shape[2:]) == (3, 3):
        _register_derived(weight, f"tap:{cd}:{c0}:{c1}", cd, REPACK_TAPS, c0, weight.shape[1] if c1 is None else c1)
    return cached((weight,), f"tap:{cd}:{c0}:{c1}", build)


def slice_weight(weight: Tensor, cd: torch.dtype, c0: int, c1: int) -> Tensor:
    """[N, 9 * (c1 - c0)] GEMM operand of a 3x3 conv parameter restricted to the input channels c0:c1 (one level of a concat)."""
    def build():
        n, c = weight.shape[0], weight.shape[1]
        w = conv_weight_matrix(weight).view(n, 9, c)[:, :, c0:c1].reshape(n, -1).contiguous()
        return w if cd == torch.float32 else ops.cast(w, cd)
    if tuple(weight.shape[2:]) == (3, 3):
        _register_derived(weight, f"slice:{cd}:{c0}:{c1}", cd, REPACK_SLICE, c0, c1)
    return cached((weight,), f"slice:{cd}:{c0}:{c1}", build)


# ------------------------------------------------------------------ conv -> BN -> ReLU
# messages of the SyncBatchNorm exchange since the last reset: [forward all-reduces, backward all-reduces]
SYNC_MESSAGES = [0, 0]


def _cba_conv(x, weight, cb, pad, up4, sync_group, running_mean, running_var, momentum):
    """conv(+bias) of a training ConvModule on NHWC x (the resize of an `up4` member fused in) -> (y, (mean, var) | None):
    the batch statistics come with y when the producing kernel emits them (gather-sum of the low-resolution forward)."""
    cd = x.dtype
    n, c, r, s = weight.shape
    if up4 and FUSE_TAPSUM and ops.resize_conv3x3_fwd_ok((x.shape[1], x.shape[2]), (up4 * x.shape[1], up4 * x.shape[2]), x.shape[0]):
        # conv3x3(resize(x)) = sum_t shift_t(resize(W_t x)): nine tap products as ONE 1x1 convolution over the
        # LOW-resolution pixels (1 / up4^2 of the MACs), then one gather-sum pass writes the full-resolution output
        z, size = ops.conv_gemm(x, tap_weight(weight, cd)), (up4 * x.shape[1], up4 * x.shape[2])
        if FUSE_TAPSUM_STATS and ops.resize_conv3x3_fwd_bn_ok(cd, n, cb):
            # ... and the batch statistics of the output come out of the same pass (per-block partial sums)
            own = _sync_world(sync_group) == 1
            y, mean, var = ops.resize_conv3x3_fwd_sum_bn([z], size, addvec=cb, running_mean=running_mean if own else None,
                                                         running_var=running_var if own else None, momentum=momentum)
            return y, (mean, var)
        return ops.resize_conv3x3_fwd_sum([z], size, addvec=cb), None
    if up4 == 4:   # conv3x3(bilinear_x4(x)) without the upsampled intermediate (ops.up4_conv3x3)
        return ops.up4_conv3x3(x, subpix4_weight(weight, cd), bias=cb), None
    if up4:        # other resize factors: the upsampled map is a temporary of the forward only (backward works on x)
        return ops.conv_gemm(ops.bilinear(x, (up4 * x.shape[1], up4 * x.shape[2])), gemm_weight(weight, cd), R=r, S=s, pad=pad,
                             bias=cb), None
    small = _sync_world(sync_group) == 1 and x.dim() == 4 and ops.BN_SMALL_MAX_PIXELS > 0 and \
        x.shape[0] * ((x.shape[1] + 2 * pad - r) + 1) * ((x.shape[2] + 2 * pad - s) + 1) <= ops.BN_SMALL_MAX_PIXELS
    if FUSE_CONV_STATS and cd == torch.bfloat16 and not small:     # (small maps: the whole BatchNorm is ONE launch, ops.bn_small_fwd)
        # the batch statistics as a side output of the convolution's epilogue (per-wave partial sums of the bf16 outputs)
        # wherever the launch is made of whole tiles on the coalesced-epilogue kernels: no statistics pass over y
        y, partials, rows = ops.conv_gemm(x, gemm_weight(weight, cd), R=r, S=s, pad=pad, bias=cb, want_stats=True)
        if not rows:
            return y, None
        own = _sync_world(sync_group) == 1
        return y, ops.bn_stats_finalize(partials, rows, n, y.numel() // n, running_mean if own else None,
                                        running_var if own else None, momentum)
    return ops.conv_gemm(x, gemm_weight(weight, cd), R=r, S=s, pad=pad, bias=cb), None


FUSE_CONV_STATS = os.environ.get("GDL_CONV_STATS", "1") != "0"   # A/B switch: False / GDL_CONV_STATS=0 = a separate statistics pass over every convolution output (round 3)


# A/B switch, OFF by default: measured SLOWER than the two launches it replaces (round 5, same-box A/B, profiles/r05a_*: 881-883
# vs 890-892 train tiles/s).  The gather's windows overlap 3.4x (10 x 22 output pixels staged per 4 x 16 footprint): the LDS-DMA
# re-reads them from L2 for free, the register-staged BN form recomputes ~10 VALU operations per element 3.4 times with two
# waves per SIMD and no DMA overlap.  Kept with its parity test as the measured reference for that design.
FUSE_BN_BWD_GATHER = os.environ.get("GDL_FUSE_BN_BWD_GATHER", "0") == "1"


def _bn_bwd_and_grads(x, weight, y, gout, mean, var, g, b, eps, relu, sg, sb, p_local, pad, up4, need_dx, need_dw):
    """BatchNorm(+ReLU) backward of a training ConvModule followed by its convolution's gradients.  For the resized 3x3
    members (up4) the BN backward is formed inside the gather kernel that consumes it (round 5: one HBM pass instead of
    bn_bwd_dx's three + the gather's read); everything else writes dy in place of y and hands it to _cba_grads."""
    if (up4 and FUSE_BN_BWD_GATHER and (need_dx or need_dw) and y.dim() == 4 and gout.is_contiguous()
            and ops.resize_conv3x3_bwd_gather_bn_ok(gout, (x.shape[1], x.shape[2]))):
        maps = ops.resize_conv3x3_bwd_gather_bn(gout, y, (x.shape[1], x.shape[2]), mean, var, g, b, eps, relu, sg, sb, p_local)
        return _cba_grads(x, weight, None, pad, up4, need_dx, need_dw, maps=maps)
    dy = ops.bn_bwd_dx(y, gout, mean, var, g, b, eps, relu, sg, sb, p_local, out=y)
    return _cba_grads(x, weight, dy, pad, up4, need_dx, need_dw)


def _cba_grads(x, weight, dy, pad, up4, need_dx, need_dw, maps=None):
    """(dx, dw) of the conv of a training ConvModule from the gradient dy of its output (BatchNorm backward already applied)."""
    n, c, r, s = weight.shape
    dx = dw = None
    if up4:
        # both gradients as GEMMs over the LOW-resolution pixels: the resize and the tap shifts act on pixels, the
        # weights on channels, so dx = sum_t W_t^T G_t and dW_t = sum_q G_t[q] (x) x[q] with G_t = resize^T shift_t^T dy
        # (ops.resize_conv3x3_bwd): 1/16 of the MACs of the full-resolution data gradient + phase weight gradients
        dx, dw = ops.resize_conv3x3_bwd(x, dy, dgrad_weight(weight, x.dtype) if need_dx else None, want_dw=need_dw, g=maps)
    else:
        if need_dx:
            dx = ops.conv_gemm(dy, dgrad_weight(weight, x.dtype), R=r, S=s, pad=r - 1 - pad)
        if need_dw:
            dw = ops.conv_wgrad(x, dy, R=r, S=s, pad=pad)
    if dw is not None:
        # same strides as the channels-last parameter (for 1x1 kernels torch keeps (C,1,1,1))
        dw = dw.view(n, c, 1, 1) if r == 1 and s == 1 else dw.view(n, r, s, c).permute(0, 3, 1, 2)
    return dx, dw


class _ConvBNActTrain(Function):
    """Training-mode ConvModule: conv(+bias) -> BatchNorm(batch stats) -> ReLU.

    Reference: models/utils.py:10-52, multilevel_neck.py:28-67 with nn.BatchNorm2d /
    nn.SyncBatchNorm semantics.
    """

    @staticmethod
    def forward(ctx, x, weight, conv_bias, gamma, beta, running_mean, running_var, momentum, eps,
                pad, relu, sync_group, up4=False):
        n = weight.shape[0]
        cb = None if conv_bias is None else conv_bias.detach()
        y, stats_done = _cba_conv(x, weight, cb, pad, up4, sync_group, running_mean, running_var, momentum)
        g, b = gamma.detach(), beta.detach()
        if _sync_world(sync_group) == 1 and stats_done is None and ops.bn_small_ok(y):
            # a small map (the reference's own per-GPU batch of 4 makes most decoder layers small): statistics, running
            # estimates and the normalised output in ONE launch
            out, mean, var = ops.bn_small_fwd(y, g, b, eps, relu, running_mean, running_var, momentum)
            _mark_running(running_mean, running_var)
            world, p_local, p_share = 1, y.numel() // n, None
        else:
            mean, var, world, p_local, p_share, _ = _bn_train_stats(y, n, running_mean, running_var, momentum, sync_group, stats_done)
            out = ops.bn_apply(y, mean, var, g, b, eps, relu)
        ctx.save_for_backward(x, weight, y, mean, var, gamma, beta)
        ctx.cfg = (pad, relu, eps, conv_bias is not None, sync_group, world, p_local, p_share, up4)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, weight, y, mean, var, gamma, beta = ctx.saved_tensors
        pad, relu, eps, has_bias, sync_group, world, p_local, p_share, up4 = ctx.cfg
        n = weight.shape[0]
        if gout.dtype != y.dtype:
            gout = to_compute(gout, y.dtype)
        g, b = gamma.detach(), beta.detach()
        if world == 1 and ops.bn_small_ok(y) and not (up4 and FUSE_BN_BWD_GATHER):
            # small map: sums, parameter gradients and dy (written over y) in ONE launch
            dy, dgamma, dbeta = ops.bn_small_bwd(y, gout, mean, var, g, b, eps, relu, out=y)
            dbias = torch.zeros(n, device=x.device, dtype=torch.float32) if has_bias and ctx.needs_input_grad[2] else None
            dx, dw = _cba_grads(x, weight, dy, pad, up4, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
            return dx, dw, dbias, dgamma, dbeta, None, None, None, None, None, None, None, None
        dgamma, dbeta = ops.bn_bwd_reduce(y, gout, mean, var, g, b, eps, relu)
        sg, sb = _bn_sync_sums(dgamma, dbeta, sync_group, world, p_share)
        dbias = None
        if has_bias and ctx.needs_input_grad[2]:
            # a bias feeding train-mode BN has an analytically zero gradient
            dbias = torch.zeros(n, device=x.device, dtype=torch.float32)
        dx, dw = _bn_bwd_and_grads(x, weight, y, gout, mean, var, g, b, eps, relu, sg, sb, p_local, pad, up4,
                                   ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dx, dw, dbias, dgamma, dbeta, None, None, None, None, None, None, None, None


class _ConvBNActGroupTrain(Function):
    """K independent training ConvModules (conv -> SyncBatchNorm(batch stats) -> ReLU on K different inputs) as ONE autograd
    node, so that their statistics cross the ranks in ONE all-reduce forward (all members' [count * mean, count * E[x^2],
    count]) and ONE backward (all members' [sum dy, sum dy * xhat]) instead of K each: the four lateral / four 3x3
    convolutions of MultiLevelNeck (multilevel_neck.py:141-160), UperNet's laterals + PPM branches + auxiliary head
    convolution (upernet.py:103-127) and its three fpn_convs (:137-141) are siblings -- 21 + 21 latency-bound messages per
    step become 6 + 6.  Per member the arithmetic is _ConvBNActTrain's; autograd runs this node's backward once all K
    output gradients exist.  flat = K x (x, weight, conv_bias, gamma, beta, running_mean, running_var)."""

    @staticmethod
    def forward(ctx, metas, sync_group, *flat):
        k = len(metas)
        mem = [flat[7 * i:7 * i + 7] for i in range(k)]
        ys, locals_, counts = [], [], []
        for (x, weight, conv_bias, gamma, beta, rm, rv), (momentum, eps, pad, relu, up4) in zip(mem, metas):
            cb = None if conv_bias is None else conv_bias.detach()
            y, stats_done = _cba_conv(x, weight, cb, pad, up4, sync_group, rm, rv, momentum)
            ys.append(y)
            locals_.append(_bn_local_stats(y, stats_done))
            counts.append(y.numel() // weight.shape[0])
        # one message: per member [n * (mean - r), n * E[(x - r)^2], n] about its running_mean r  (count-weighted merge, see sync_batch_stats)
        fused = FUSE_SYNC_MESSAGE and ys[0].is_cuda
        pivots = [_sync_pivot(m[5], m[1].shape[0]) for m in mem]
        for piv in pivots:
            check_sync_pivot(piv, sync_group or None)
        if fused:      # every member packs its share straight into its slice of the message: no torch arithmetic, no cat
            packed = torch.empty(sum(2 * w.shape[0] + 1 for (_, w, *_r) in mem), device=ys[0].device, dtype=torch.float32)
            off = 0
            for (mean, var), n, piv in zip(locals_, counts, pivots):
                ops.syncbn_pack(mean, var, float(n), packed[off:off + 2 * mean.numel() + 1], piv)
                off += 2 * mean.numel() + 1
        else:
            packed = torch.cat([t for (mean, var), n, piv in zip(locals_, counts, pivots) for t in sync_message(mean, var, float(n), piv)])
        dist.all_reduce(packed, group=sync_group or None)
        SYNC_MESSAGES[0] += 1
        outs, saved, cfg, off = [], [], [], 0
        for (x, weight, conv_bias, gamma, beta, rm, rv), (momentum, eps, pad, relu, up4), y, n, piv in zip(mem, metas, ys, counts, pivots):
            c = weight.shape[0]
            total = packed[off + 2 * c]
            if fused:  # global statistics + the running-estimate update in one kernel (it reads the pivot, rm, before it writes rm)
                gmean, gvar = ops.syncbn_unpack(packed[off:off + 2 * c + 1], c, rm, rv, momentum, pivot=piv)
                _mark_running(rm, rv)
            else:
                gmean, gvar, _ = sync_message_stats(packed[off:off + 2 * c + 1], c, piv)
                if rm is not None:
                    update_running_stats(rm, rv, gmean, gvar, momentum, total)
            off += 2 * c + 1
            outs.append(ops.bn_apply(y, gmean, gvar, gamma.detach(), beta.detach(), eps, relu))
            saved += [x, weight, y, gmean, gvar, gamma, beta]
            cfg.append((pad, relu, eps, conv_bias is not None, n, (total if fused else n / total), up4))
        ctx.fused_message = fused
        ctx.save_for_backward(*saved)
        ctx.cfg, ctx.sync_group = cfg, sync_group
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        k = len(ctx.cfg)
        mem = [ctx.saved_tensors[7 * i:7 * i + 7] for i in range(k)]
        sums = []
        gs = []
        for (x, weight, y, mean, var, gamma, beta), (pad, relu, eps, has_bias, p_local, p_share, up4), gout in zip(mem, ctx.cfg, gouts):
            if gout.dtype != y.dtype:
                gout = to_compute(gout, y.dtype)
            gs.append(gout)
            sums.append(ops.bn_bwd_reduce(y, gout, mean, var, gamma.detach(), beta.detach(), eps, relu))
        packed = torch.cat([t for pair in sums for t in pair])
        dist.all_reduce(packed, group=ctx.sync_group or None)
        SYNC_MESSAGES[1] += 1
        grads, off = [], 0
        for i, ((x, weight, y, mean, var, gamma, beta), (pad, relu, eps, has_bias, p_local, p_share, up4), gout, (dgamma, dbeta)) in \
                enumerate(zip(mem, ctx.cfg, gs, sums)):
            c = weight.shape[0]
            need = ctx.needs_input_grad[2 + 7 * i:2 + 7 * i + 7]
            if ctx.fused_message:
                # p_share holds the GLOBAL count (a device scalar: the count entry of the forward message): the backward-dx kernel
                # divides the all-reduced sums by it itself -- no scaling launches, the message slices are used in place
                dy = ops.bn_bwd_dx_sync(y, gout, mean, var, gamma.detach(), beta.detach(), eps, relu, packed[off:off + c],
                                        packed[off + c:off + 2 * c], p_share.reshape(1), out=y)
                dx, dw = _cba_grads(x, weight, dy, pad, up4, need[0], need[1])
            else:
                sg, sb = packed[off:off + c] * p_share, packed[off + c:off + 2 * c] * p_share
                dx, dw = _bn_bwd_and_grads(x, weight, y, gout, mean, var, gamma.detach(), beta.detach(), eps, relu, sg.contiguous(),
                                           sb.contiguous(), p_local, pad, up4, need[0], need[1])
            off += 2 * c
            dbias = torch.zeros(c, device=x.device, dtype=torch.float32) if has_bias and need[2] else None
            grads += [dx, dw, dbias, dgamma, dbeta, None, None]
        return (None, None, *grads)


def conv_bn_act_group(items: list[dict]) -> list[Tensor]:
    """[conv_bn_act(**item) for item in items] for INDEPENDENT ConvModules (item: x, conv, norm, relu, up).  Under
    SyncBatchNorm training with more than one rank the members share one statistics message per direction
    (_ConvBNActGroupTrain); otherwise they simply run one after the other."""
    norms = [it["norm"] for it in items]
    grouped = (GROUP_SYNC_BN and len(items) > 1 and all(isinstance(nm, nn.SyncBatchNorm) and nm.training for nm in norms)
               and len({id(nm.process_group) for nm in norms}) == 1 and _world(norms[0].process_group) > 1)
    if grouped:
        for it in items:      # members the single-module path would have re-routed (odd shapes) keep that path
            conv, x, up = it["conv"], it["x"], int(it.get("up", 1))
            if up > 1 and not (conv.kernel_size[0] == 3 and conv.padding[0] == 1 and x.shape[1] >= 2 and x.shape[2] >= 2
                               and FUSE_UP4 and conv.weight.shape[0] % 8 == 0 and x.shape[0] * x.shape[1] <= 65535 and up in (2, 4)):
                grouped = False
    if not grouped:
        return [conv_bn_act(it["x"], it["conv"], it["norm"], relu=it.get("relu", True), up=it.get("up", 1)) for it in items]
    metas, flat = [], []
    for it in items:
        conv, norm = it["conv"], it["norm"]
        metas.append((_bn_sync_momentum(norm)[1], norm.eps, conv.padding[0], it.get("relu", True), int(it.get("up", 1)) if it.get("up", 1) > 1 else 0))
        flat += [it["x"], conv.weight, conv.bias, norm.weight, norm.bias, norm.running_mean, norm.running_var]
    outs = _ConvBNActGroupTrain.apply(tuple(metas), norms[0].process_group, *flat)
    for norm in norms:
        bump(norm.num_batches_tracked)
    return list(outs)


GROUP_SYNC_BN = True   # A/B switch: False = one statistics exchange per ConvModule (round 2)


FUSE_CONCAT_BWD = True   # A/B switch: False = keep the concat buffer and run the full-resolution data / weight gradients


def _concat_resize_conv(weight, levels):
    """(y, chans): the 3x3 convolution of _ConcatResizeConvBNTrain over the concat of the resized levels, before BatchNorm."""
    cd = levels[0].dtype
    B, H, W, _ = levels[0].shape
    chans = [lv.shape[3] for lv in levels]
    if _tapsum_levels_ok(levels):
        # per level (the convolution is linear over the concat): the native level runs the 3x3 kernel on its own
        # channel slice; every upsampled level contributes its nine tap products, computed at ITS resolution, through
        # one gather-sum pass whose result enters the native level's GEMM as the residual operand
        offs = [sum(chans[:j]) for j in range(len(chans))]
        zs = [ops.conv_gemm(lv, tap_weight(weight, cd, o, o + c)) for lv, o, c in zip(levels[1:], offs[1:], chans[1:])]
        y = ops.conv_gemm(levels[0], slice_weight(weight, cd, 0, chans[0]), R=3, S=3, pad=1,
                          resid=ops.resize_conv3x3_fwd_sum(zs, (H, W)))
        del zs
    else:
        cat = torch.empty((B, H, W, sum(chans)), device=levels[0].device, dtype=cd)
        off = 0
        for lv, c in zip(levels, chans):
            ops.bilinear(lv, (H, W), out=cat[..., off:off + c])
            off += c
        y = ops.conv_gemm(cat, gemm_weight(weight, cd), R=3, S=3, pad=1)
        del cat
    return y, chans


def _concat_resize_conv_grads(weight, dy, levels, chans, want_dw, need_dxs):
    """(dw, [d level_j]) of _concat_resize_conv from the gradient dy of its output."""
    n, ctot = weight.shape[0], weight.shape[1]
    H, W = dy.shape[1], dy.shape[2]
    wd = dgrad_weight(weight, dy.dtype)                        # [sum(C_j), 9 N]: the rows of a level are contiguous
    dw = torch.empty((n, 9, ctot), device=dy.device, dtype=torch.float32) if want_dw else None
    dls, off = [], 0
    for j, (lv, c) in enumerate(zip(levels, chans)):
        need_dx = need_dxs[j]
        if (lv.shape[1], lv.shape[2]) == (H, W):
            dls.append(ops.conv_gemm(dy, wd[off:off + c], R=3, S=3, pad=1) if need_dx else None)
            if want_dw:
                dw[:, :, off:off + c] = ops.conv_wgrad(lv, dy, R=3, S=3, pad=1).view(n, 9, c)
        else:
            dx, dwl = ops.resize_conv3x3_bwd(lv, dy, wd[off:off + c] if need_dx else None, want_dw=want_dw)
            dls.append(dx)
            if want_dw:
                dw[:, :, off:off + c] = dwl.view(n, 9, c)
        off += c
    if want_dw:
        dw = dw.view(n, 3, 3, ctot).permute(0, 3, 1, 2)
    return dw, dls


class _ConcatResizeConvBNTrain(Function):
    """conv3x3(pad 1)(cat([l_0, bilinear(l_1 -> size), ..., bilinear(l_k -> size)])) -> BatchNorm(batch stats) -> ReLU
    (UperNet `fpn_bottleneck` over the upsampled FPN levels, upernet.py:144-152).  Forward: the levels are resized straight
    into the concat buffer and ONE K = 9 * sum(C_j) convolution runs on it; the buffer is a temporary.  Backward, per level:
    the native-resolution level gets its slice of the ordinary data / weight gradient; an upsampled level gets both as GEMMs
    over ITS OWN pixels from the nine gathered maps G_t = resize^T shift_t^T dy (ops.resize_conv3x3_bwd_gather) -- 1/4,
    1/16, 1/64 of the MACs, no bilinear backward, and neither the concat buffer nor its gradient exists in backward."""

    @staticmethod
    def forward(ctx, weight, gamma, beta, running_mean, running_var, momentum, eps, relu, sync_group, *levels):
        n = weight.shape[0]
        y, chans = _concat_resize_conv(weight, levels)
        mean, var, world, p_local, p_share, _ = _bn_train_stats(y, n, running_mean, running_var, momentum, sync_group)
        out = ops.bn_apply(y, mean, var, gamma.detach(), beta.detach(), eps, relu)
        ctx.save_for_backward(weight, y, mean, var, gamma, beta, *levels)
        ctx.cfg = (relu, eps, sync_group, world, p_local, p_share, chans)
        return out

    @staticmethod
    def backward(ctx, gout):
        weight, y, mean, var, gamma, beta, *levels = ctx.saved_tensors
        relu, eps, sync_group, world, p_local, p_share, chans = ctx.cfg
        dy, dgamma, dbeta = _bn_train_backward(y, gout, mean, var, gamma.detach(), beta.detach(), eps, relu, sync_group,
                                               world, p_local, p_share)
        dw, dls = _concat_resize_conv_grads(weight, dy, levels, chans, ctx.needs_input_grad[0], ctx.needs_input_grad[9:])
        return (dw, dgamma, dbeta, None, None, None, None, None, None, *dls)


# A/B switch: 0 = the decoder tail runs bn_apply -> head and head backward -> BatchNorm backward as separate launches
FUSE_BN_TAIL = os.environ.get("GDL_FUSE_BN_TAIL", "1") != "0"


class _ConcatResizeConvBNHeadTrain(Function):
    """_ConcatResizeConvBNTrain and the 1x1 classifier head on its output as ONE node (bf16, single-process statistics): the
    head is the only consumer of z = ReLU(BN(y)) in a training step, its gradient dz = dlogits . W is five multiply-adds per
    element of a tensor 1 / 50 the size of the map, and z is one f32 expression of the saved convolution output y.  So neither
    z nor dz is ever written: the head forms z from y on load (ops.head_1x1_bn, bit-identical logits), the backward forms z
    and dz from y and dlogits inside the BatchNorm sums pass -- which also accumulates the head's dW / db -- and inside the
    dx pass (ops.bn_head_bwd_reduce / bn_head_bwd_dx).  Output: the head's [B, H, W, K] f32 logits."""

    @staticmethod
    def forward(ctx, weight, gamma, beta, running_mean, running_var, momentum, eps, relu, head_w, head_b, *levels):
        n = weight.shape[0]
        y, chans = _concat_resize_conv(weight, levels)
        mean, var, _, p_local, _, _ = _bn_train_stats(y, n, running_mean, running_var, momentum, False)
        low = ops.head_1x1_bn(y, mean, var, gamma.detach(), beta.detach(), eps, relu, head_w.detach(),
                              None if head_b is None else head_b.detach())
        ctx.save_for_backward(weight, y, mean, var, gamma, beta, head_w, *levels)
        ctx.cfg = (relu, eps, p_local, chans, head_b is not None)
        return low

    @staticmethod
    def backward(ctx, dlow):
        weight, y, mean, var, gamma, beta, head_w, *levels = ctx.saved_tensors
        relu, eps, p_local, chans, has_bias = ctx.cfg
        dlow = dlow.contiguous()
        g, b, hw = gamma.detach(), beta.detach(), head_w.detach()
        dgamma, dbeta, dhw, dhb = ops.bn_head_bwd_reduce(y, dlow, hw, mean, var, g, b, eps, relu)
        dy = ops.bn_head_bwd_dx(y, dlow, hw, mean, var, g, b, eps, relu, dgamma, dbeta, p_local, out=y)
        dw, dls = _concat_resize_conv_grads(weight, dy, levels, chans, ctx.needs_input_grad[0], ctx.needs_input_grad[10:])
        return (dw, dgamma, dbeta, None, None, None, None, None, dhw.view(head_w.shape), dhb if has_bias else None, *dls)


def bn_tail_fusable(y_shape, dtype: torch.dtype, norm: nn.Module, head_conv: nn.Conv2d) -> bool:
    """Shapes / modes the fused BatchNorm + head tail takes: bf16, train-mode statistics of ONE process, a dense 256-channel
    map and a 1x1 head of at most 8 classes with f32 parameters (gdl_head_1x1_bn_ok / gdl_bn_head_bwd_ok)."""
    if not (FUSE_BN_TAIL and norm.training and dtype == torch.bfloat16 and torch.is_grad_enabled()):
        return False
    if not single_process_bn_train(norm):
        return False
    hw = head_conv.weight
    if head_conv.kernel_size != (1, 1) or hw.dtype != torch.float32 or not hw.is_contiguous() or hw.shape[1] != y_shape[3]:
        return False
    P, C, K = y_shape[0] * y_shape[1] * y_shape[2], y_shape[3], hw.shape[0]
    lib = ops._lib.load()
    return bool(lib.gdl_head_1x1_bn_ok(ops.BF16, P, C, K)) and bool(lib.gdl_bn_head_bwd_ok(ops.BF16, P, C, K))


def _tapsum_levels_ok(levels) -> bool:
    """levels[0] native, 1..3 further levels each upsampled: by an integer factor of 2 / 4 / 8 (one pass for all of them) or by
    any other ratio up to 10 (one plain gather pass each) -- ops.resize_conv3x3_fwd_sum."""
    B, H, W, _ = levels[0].shape
    return (FUSE_TAPSUM and 2 <= len(levels) <= 4
            and all(ops.resize_conv3x3_fwd_ok((lv.shape[1], lv.shape[2]), (H, W), B)
                    or ops.resize_conv3x3_any_ok((lv.shape[1], lv.shape[2]), (H, W), B) for lv in levels[1:]))


def concat_resize_conv_bn_act(levels: list[Tensor], conv: nn.Conv2d, norm: nn.Module, *, relu: bool = True,
                              head_conv: nn.Conv2d | None = None) -> Tensor:
    """ConvModule(3x3, pad 1, no bias) over cat([levels[0]] + [bilinear(l -> levels[0]'s size) for l in levels[1:]]) on NHWC
    maps.  Training: see _ConcatResizeConvBNTrain; eval (and resize factors above 8): concat_upsample + conv_bn_act.
    ``head_conv``: the caller has checked bn_tail_fusable() and wants the [B, H, W, K] f32 logits of that 1x1 head over the
    result instead of the result (_ConcatResizeConvBNHeadTrain); when the fused training node does not apply the head runs
    on the materialised map (_Head1x1)."""
    size = (levels[0].shape[1], levels[0].shape[2])
    def factor_ok(lv):
        fy, fx = size[0] / lv.shape[1], size[1] / lv.shape[2]
        return (lv.shape[1], lv.shape[2]) == size or (1.0 < fy <= ops.MAX_ANY_RESIZE and 1.0 < fx <= ops.MAX_ANY_RESIZE)
    ok = (FUSE_CONCAT_BWD and norm.training and conv.kernel_size == (3, 3) and conv.padding == (1, 1) and conv.bias is None
          and conv.weight.shape[0] % 8 == 0 and all(lv.is_contiguous() and factor_ok(lv) for lv in levels)
          and levels[0].shape[0] * max(lv.shape[1] for lv in levels) <= 65535)
    if (not norm.training and conv.kernel_size == (3, 3) and conv.padding == (1, 1) and conv.bias is None
            and all(lv.is_contiguous() for lv in levels) and _tapsum_levels_ok(levels)
            and not (torch.is_grad_enabled() and (conv.weight.requires_grad or any(lv.requires_grad for lv in levels)))):
        # eval, per level: folded BatchNorm scale in every weight slice, epilogue relu(acc + shift + gather-sum)
        cd = levels[0].dtype
        chans = [lv.shape[3] for lv in levels]

        def fold():
            scale, shift = ops.bn_fold(norm.weight.detach(), norm.bias.detach(), norm.running_mean, norm.running_var, norm.eps)
            n, c = conv.weight.shape[0], conv.weight.shape[1]
            w = conv_weight_matrix(conv.weight).float().view(n, 9, c) * scale[:, None, None]
            cast = (lambda t: t) if cd == torch.float32 else (lambda t: ops.cast(t, cd))
            w0 = cast(w[:, :, :chans[0]].reshape(n, -1).contiguous())
            taps, off = [], chans[0]
            for cj in chans[1:]:
                taps.append(cast(w[:, :, off:off + cj].permute(1, 0, 2).reshape(9 * n, cj).contiguous()))
                off += cj
            return w0, taps, shift
        w0, taps, shift = cached((conv.weight, norm.weight, norm.bias, norm.running_mean, norm.running_var),
                                 f"catfold:{cd}:{chans}", fold)
        zs = [ops.conv_gemm(lv, wt) for lv, wt in zip(levels[1:], taps)]
        return ops.conv_gemm(levels[0], w0, R=3, S=3, pad=1, bias=shift, resid=ops.resize_conv3x3_fwd_sum(zs, size),
                             act=ACT_RESID_RELU if relu else ACT_NONE)
    if not ok:
        if FUSE_CONCAT_BWD and norm.training:
            warn_unfused("3x3 ConvModule over a concat of resized levels", f"levels {[tuple(lv.shape) for lv in levels]}: needs "
                         "contiguous levels, resize factors <= 10, N % 8 == 0 and batch * rows <= 65535")
        out = conv_bn_act(concat_upsample(levels, size), conv, norm, relu=relu)
        return out if head_conv is None else _Head1x1.apply(out, head_conv.weight, head_conv.bias, None)
    sync_group, momentum = _bn_sync_momentum(norm)
    if head_conv is not None:
        low = _ConcatResizeConvBNHeadTrain.apply(conv.weight, norm.weight, norm.bias, norm.running_mean, norm.running_var, momentum,
                                                 norm.eps, relu, head_conv.weight, head_conv.bias, *levels)
        bump(norm.num_batches_tracked)
        return low
    out = _ConcatResizeConvBNTrain.apply(conv.weight, norm.weight, norm.bias, norm.running_mean, norm.running_var, momentum,
                                         norm.eps, relu, sync_group, *levels)
    bump(norm.num_batches_tracked)
    return out


FUSE_PYRAMID = True   # A/B switch: False = upsample every level into a concat buffer and run one wide 1x1 convolution


class _PyramidFuseBNTrain(Function):
    """conv1x1(cat([bilinear(l_0 -> size), ..., bilinear(l_{k-1} -> size), l_k])) -> BatchNorm(batch stats) -> ReLU
    (segformer_mlp.py:97-125 `linear_fuse`), evaluated PER LEVEL: a 1x1 convolution acts per pixel and a bilinear resize
    per channel, so they commute -- W_j is applied to level j at the level's own resolution (1/4, 1/16, 1/64 of the
    pixels), the small results are upsampled and summed in one pass (ops.bilinear_sum) and enter the last level's GEMM as
    its residual operand.  Neither the upsampled levels nor the concat buffer exist; forward, data-gradient and
    weight-gradient GEMMs shrink from K = sum(E_j) at full resolution to one K = E_k GEMM at full resolution plus small
    ones.  Backward: dz_j = bilinear^T(dy) per level, then the level's own dgrad / wgrad."""

    @staticmethod
    def forward(ctx, weight, gamma, beta, running_mean, running_var, momentum, eps, relu, sync_group, *levels):
        cd = levels[0].dtype
        n = weight.shape[0]
        wq = gemm_weight(weight, cd)
        size = (levels[-1].shape[1], levels[-1].shape[2])
        offs, off = [], 0
        for lv in levels:
            offs.append(off)
            off += lv.shape[3]
        zs = [ops.conv_gemm(lv, wq[:, o:o + lv.shape[3]]) for lv, o in zip(levels[:-1], offs[:-1])]
        y = ops.conv_gemm(levels[-1], wq[:, offs[-1]:], resid=ops.bilinear_sum(zs, size))
        mean, var, world, p_local, p_share, _ = _bn_train_stats(y, n, running_mean, running_var, momentum, sync_group)
        out = ops.bn_apply(y, mean, var, gamma.detach(), beta.detach(), eps, relu)
        ctx.save_for_backward(weight, y, mean, var, gamma, beta, *levels)
        ctx.cfg = (relu, eps, sync_group, world, p_local, p_share, offs)
        return out

    @staticmethod
    def backward(ctx, gout):
        weight, y, mean, var, gamma, beta, *levels = ctx.saved_tensors
        relu, eps, sync_group, world, p_local, p_share, offs = ctx.cfg
        n, ctot = weight.shape[0], weight.shape[1]
        cd = y.dtype
        dy, dgamma, dbeta = _bn_train_backward(y, gout, mean, var, gamma.detach(), beta.detach(), eps, relu, sync_group,
                                               world, p_local, p_share)
        dzs = [ops.bilinear_bwd(dy, (lv.shape[1], lv.shape[2])) for lv in levels[:-1]] + [dy]
        wd = dgrad_weight(weight, cd)                       # [sum(E_j), N]: rows of level j are contiguous
        dls = []
        for j, (lv, dz, o) in enumerate(zip(levels, dzs, offs)):
            dls.append(ops.conv_gemm(dz, wd[o:o + lv.shape[3]]) if ctx.needs_input_grad[9 + j] else None)
        dw = None
        if ctx.needs_input_grad[0]:
            dw = torch.empty((n, ctot), device=y.device, dtype=torch.float32)
            for lv, dz, o in zip(levels, dzs, offs):
                ops.conv_wgrad(lv, dz, R=1, S=1, dw=dw[:, o:o + lv.shape[3]])
            dw = dw.view(n, ctot, 1, 1)
        return (dw, dgamma, dbeta, None, None, None, None, None, None, *dls)


def pyramid_fuse_bn_act(levels: list[Tensor], conv: nn.Conv2d, norm: nn.Module, *, relu: bool = True) -> Tensor:
    """ConvModule(1x1, no bias) over cat([bilinear(l -> size of levels[-1]) for l in levels[:-1]] + [levels[-1]]) on NHWC
    maps, without the concat (see _PyramidFuseBNTrain).  Eval mode: the folded BN scale goes into the weights, so that every
    level's partial result is already scaled and the last GEMM's epilogue is relu(acc + shift + residual)."""
    ok = (FUSE_PYRAMID and conv.kernel_size == (1, 1) and conv.bias is None and 2 <= len(levels) <= 4
          and all(lv.is_contiguous() for lv in levels) and levels[-1].shape[0] * levels[-1].shape[1] <= 65535)
    size = (levels[-1].shape[1], levels[-1].shape[2])
    if not ok:
        if FUSE_PYRAMID:
            warn_unfused("1x1 ConvModule over a concat of resized levels", f"levels {[tuple(lv.shape) for lv in levels]}: needs 2..4 "
                         "contiguous levels, no bias and batch * rows <= 65535")
        return conv_bn_act(concat_upsample(levels, size), conv, norm, relu=relu)
    if norm.training:
        sync_group, momentum = _bn_sync_momentum(norm)
        out = _PyramidFuseBNTrain.apply(conv.weight, norm.weight, norm.bias, norm.running_mean, norm.running_var,
                                        momentum, norm.eps, relu, sync_group, *levels)
        bump(norm.num_batches_tracked)
        return out
    if torch.is_grad_enabled() and (conv.weight.requires_grad or any(lv.requires_grad for lv in levels)):
        raise NotImplementedError(_EVAL_BN_GRAD_MSG)
    cd = levels[0].dtype

    def fold():
        scale, shift = ops.bn_fold(norm.weight.detach(), norm.bias.detach(), norm.running_mean, norm.running_var, norm.eps)
        w = conv_weight_matrix(conv.weight).float() * scale[:, None]
        return (w.contiguous() if cd == torch.float32 else ops.cast(w.contiguous(), cd)), shift
    wq, shift = cached((conv.weight, norm.weight, norm.bias, norm.running_mean, norm.running_var), f"pyrfold:{cd}", fold)
    off, zs = 0, []
    for lv in levels[:-1]:
        zs.append(ops.conv_gemm(lv, wq[:, off:off + lv.shape[3]]))
        off += lv.shape[3]
    return ops.conv_gemm(levels[-1], wq[:, off:], bias=shift, resid=ops.bilinear_sum(zs, size),
                         act=ACT_RESID_RELU if relu else ACT_NONE)


def subpix4_weight(weight: Tensor, cd: torch.dtype) -> dict:
    """Phase weight sets of conv3x3(bilinear_x4(.)) for a [N,C,3,3] conv parameter (cached per parameter version)."""
    def build():
        w = conv_weight_matrix(weight)
        return ops.subpix4_weights(w.float().contiguous(), weight.shape[1], cd)
    return cached((weight,), f"subpix4:{cd}", build)


def conv_bn_act(x: Tensor, conv: nn.Conv2d, norm: nn.Module, *, relu: bool = True, up4: bool = False, up: int = 1) -> Tensor:
    """ConvModule forward on an NHWC tensor (in the compute dtype); returns NHWC.  ``up`` (2 or 4; ``up4`` = 4): the input is
    bilinearly upsampled by that factor first (MultiLevelNeck's fine levels).  Factor 4 runs as sub-pixel phase convolutions
    on the low-resolution map (ops.up4_conv3x3); for both factors the BACKWARD runs at low resolution
    (ops.resize_conv3x3_bwd), the upsampled map is never kept."""
    r = conv.kernel_size[0]
    pad = conv.padding[0]
    up4 = 4 if up4 else (int(up) if up in (2, 4) else 0)      # from here on: the resize factor fused into the node (0 = none)
    if up > 1 and not up4:
        x = bilinear(x, (int(up) * x.shape[1], int(up) * x.shape[2]))
    if up4 and not (r == 3 and pad == 1 and x.shape[1] >= 2 and x.shape[2] >= 2 and FUSE_UP4 and conv.weight.shape[0] % 8 == 0
                    and x.shape[0] * x.shape[1] <= 65535):      # (the gather kernels put batch x rows in one grid dimension)
        if FUSE_UP4:
            warn_unfused(f"ConvModule on a x{up4} resized input", f"input {tuple(x.shape)}, {conv.weight.shape[0]} output channels: "
                         "needs a 3x3 / pad 1 filter, N % 8 == 0 and batch * rows <= 65535")
        x, up4 = bilinear(x, (up4 * x.shape[1], up4 * x.shape[2])), 0
    if norm.training:
        sync_group, momentum = _bn_sync_momentum(norm)
        out = _ConvBNActTrain.apply(x, conv.weight, conv.bias, norm.weight, norm.bias,
                                    norm.running_mean, norm.running_var, momentum, norm.eps, pad,
                                    relu, sync_group, up4)
        bump(norm.num_batches_tracked)
        return out
    if torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad):
        raise NotImplementedError(_EVAL_BN_GRAD_MSG)
    cd = x.dtype
    scale, shift = cached((norm.weight, norm.bias, norm.running_mean, norm.running_var), "bnfold",
                          lambda: ops.bn_fold(norm.weight.detach(), norm.bias.detach(),
                                              norm.running_mean, norm.running_var, norm.eps))
    if up4 and FUSE_TAPSUM and ops.resize_conv3x3_fwd_ok((x.shape[1], x.shape[2]), (up4 * x.shape[1], up4 * x.shape[2]),
                                                         x.shape[0]):
        # eval: the BatchNorm scale is folded into the tap weights, shift (+ scale * bias) and the ReLU into the gather-sum
        def fold():
            n, c = conv.weight.shape[0], conv.weight.shape[1]
            w = conv_weight_matrix(conv.weight).float().view(n, 9, c) * scale[:, None, None]
            w = w.permute(1, 0, 2).reshape(9 * n, c).contiguous()
            add = shift if conv.bias is None else (shift + scale * conv.bias.detach().float()).contiguous()
            return (w if cd == torch.float32 else ops.cast(w, cd)), add
        keyp = (conv.weight, norm.weight, norm.bias, norm.running_mean, norm.running_var) + (() if conv.bias is None else (conv.bias,))
        wq, add = cached(keyp, f"tapfold:{cd}", fold)
        return ops.resize_conv3x3_fwd_sum([ops.conv_gemm(x, wq)], (up4 * x.shape[1], up4 * x.shape[2]), addvec=add, relu=relu)
    if up4 == 4:
        return ops.up4_conv3x3(x, subpix4_weight(conv.weight, cd), bias=None if conv.bias is None else conv.bias.detach(),
                               scale=scale, shift=shift, act=ACT_RELU if relu else ACT_NONE)
    if up4:
        x = ops.bilinear(x, (up4 * x.shape[1], up4 * x.shape[2]))
    return ops.conv_gemm(x, gemm_weight(conv.weight, cd), R=r, S=r, pad=pad,
                         bias=None if conv.bias is None else conv.bias.detach(), scale=scale,
                         shift=shift, act=ACT_RELU if relu else ACT_NONE)


# ------------------------------------------------------------------ UperNet scale_modules (upernet.py:37-54,113-119)


def _nhwc_grad(g: Tensor, dtype: torch.dtype) -> Tensor:
    """Incoming gradient as an NHWC tensor of the node's compute dtype with unit channel stride."""
    if g.dtype != dtype:
        return to_compute(g if g.stride(-1) == 1 else g.contiguous(), dtype)
    return g if g.stride(-1) == 1 else ops.copy_cast(g.contiguous())


def _check_convt2x2(convt: nn.ConvTranspose2d) -> None:
    if not (isinstance(convt, nn.ConvTranspose2d) and tuple(convt.kernel_size) == (2, 2) and tuple(convt.stride) == (2, 2)
            and tuple(convt.padding) == (0, 0) and tuple(convt.output_padding) == (0, 0) and tuple(convt.dilation) == (1, 1)
            and convt.groups == 1):
        raise NotImplementedError(f"gdlhip: only nn.ConvTranspose2d(kernel_size=2, stride=2) without padding / groups / dilation "
                                  f"has a HIP path, got {convt}")


def convt2x2_operands(convt: nn.ConvTranspose2d, cd: torch.dtype) -> tuple[Tensor, Tensor]:
    """(forward, data-gradient) GEMM operands of a ConvTranspose2d(2, 2) parameter in the compute dtype.  A weight that is being
    trained is packed inside EVERY forward (one small launch): the operands can never be one optimizer update behind, whoever
    rewrote the parameter and through whatever pointer, and a captured step is correct by construction.  Frozen weights and eval
    go through the version-keyed cache."""
    w = convt.weight
    if w.requires_grad and convt.training and torch.is_grad_enabled():
        return ops.convt2x2_pack(w.detach(), cd)
    return cached((w,), f"convt2x2:{cd}", lambda: ops.convt2x2_pack(w.detach(), cd))


def _convt2x2_backward(x, gout, w_dgrad, need_dx, need_dw):
    dx = ops.convt2x2_dgrad(gout, w_dgrad) if need_dx else None
    dw = ops.convt2x2_wgrad(x, gout) if need_dw else None
    return dx, dw


class _ConvT2x2(Function):
    """nn.ConvTranspose2d(kernel 2, stride 2) on NHWC (upernet.py:39,42,45)."""

    @staticmethod
    def forward(ctx, x, weight, bias, w_fwd, w_dgrad):
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ctx.save_for_backward(x if need_dw else None, w_dgrad if need_dx else None)
        return ops.convt2x2(x, w_fwd, None if bias is None else bias.detach())

    @staticmethod
    def backward(ctx, gout):
        x, w_dgrad = ctx.saved_tensors
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        gout = _nhwc_grad(gout, (x if x is not None else w_dgrad).dtype) if (need_dx or need_dw) else gout
        dx, dw = _convt2x2_backward(x, gout, w_dgrad, need_dx, need_dw)
        db = ops.colsum(gout if gout.stride(-1) == 1 else gout.contiguous()) if need_db else None
        return dx, dw, db, None, None


def conv_transpose2x2(x: Tensor, convt: nn.ConvTranspose2d) -> Tensor:
    """ConvTranspose2d(kernel 2, stride 2) forward on an NHWC tensor in the compute dtype: [B,H,W,Cin] -> [B,2H,2W,Cout]."""
    _check_convt2x2(convt)
    w_fwd, w_dgrad = convt2x2_operands(convt, x.dtype)
    bias = convt.bias
    if torch.is_grad_enabled() and (x.requires_grad or convt.weight.requires_grad or (bias is not None and bias.requires_grad)):
        return _ConvT2x2.apply(x, convt.weight, bias, w_fwd, w_dgrad)
    return ops.convt2x2(x, w_fwd, None if bias is None else bias.detach())


class _ConvT2x2BNGeluTrain(Function):
    """Training-mode ConvTranspose2d(2, 2) -> BatchNorm(batch statistics) -> GELU (upernet.py:39-41), nn.BatchNorm2d /
    nn.SyncBatchNorm semantics as _ConvBNActTrain.  Saved for the backward: the input, the convolution output (overwritten by its
    gradient there) and the statistics; gelu'(bn(.)) is recomputed."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, momentum, eps, sync_group, w_fwd, w_dgrad):
        n = w_fwd.shape[1]
        y = ops.convt2x2(x, w_fwd, None if bias is None else bias.detach())
        # (the dx kernel reads the global count `total` itself: no p_share)
        mean, var, world, p_local, _, total = _bn_train_stats(y, n, running_mean, running_var, momentum, sync_group)
        out = ops.bn_gelu_apply(y, mean, var, gamma.detach(), beta.detach(), eps)
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ctx.save_for_backward(x if need_dw else None, w_dgrad if need_dx else None, y, mean, var, gamma, beta, total)
        ctx.cfg = (eps, bias is not None, sync_group, world, p_local)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, w_dgrad, y, mean, var, gamma, beta, total = ctx.saved_tensors
        eps, has_bias, sync_group, world, p_local = ctx.cfg
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gout = _nhwc_grad(gout, y.dtype)
        g, b = gamma.detach(), beta.detach()
        dgamma, dbeta = ops.bn_gelu_bwd_reduce(y, gout, mean, var, g, b, eps)
        sg, sb = _bn_sync_sums(dgamma, dbeta, sync_group, world)
        dx = dw = None
        if need_dx or need_dw:
            dy = ops.bn_gelu_bwd_dx(y, gout, mean, var, g, b, eps, sg, sb, p_local, total_count=total, out=y)
            dx, dw = _convt2x2_backward(x, dy, w_dgrad, need_dx, need_dw)
        # a bias feeding train-mode BatchNorm has an analytically zero gradient
        db = torch.zeros(y.shape[-1], device=y.device, dtype=torch.float32) if has_bias and ctx.needs_input_grad[2] else None
        return (dx, dw, db, dgamma if ctx.needs_input_grad[3] else None, dbeta if ctx.needs_input_grad[4] else None,
                None, None, None, None, None, None, None)


def conv_transpose2x2_bn_gelu(x: Tensor, convt: nn.ConvTranspose2d, norm: nn.Module) -> Tensor:
    """ConvTranspose2d(2, 2) -> BatchNorm2d -> GELU (erf) on an NHWC tensor in the compute dtype (UperNet scale_modules fpn1[0:3])."""
    _check_convt2x2(convt)
    w_fwd, w_dgrad = convt2x2_operands(convt, x.dtype)
    if norm.training:
        sync_group, momentum = _bn_sync_momentum(norm)
        out = _ConvT2x2BNGeluTrain.apply(x, convt.weight, convt.bias, norm.weight, norm.bias, norm.running_mean, norm.running_var,
                                         momentum, norm.eps, sync_group, w_fwd, w_dgrad)
        bump(norm.num_batches_tracked)
        return out
    if torch.is_grad_enabled() and (x.requires_grad or convt.weight.requires_grad):
        raise NotImplementedError(_EVAL_BN_GRAD_MSG)
    y = ops.convt2x2(x, w_fwd, None if convt.bias is None else convt.bias.detach())
    return ops.bn_gelu_apply(y, norm.running_mean, norm.running_var, norm.weight.detach(), norm.bias.detach(), norm.eps, out=y)


class _MaxPool2x2(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.maxpool2x2s2(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.maxpool2x2s2_bwd(x, _nhwc_grad(g, x.dtype))


def maxpool2x2(x: Tensor) -> Tensor:
    """nn.MaxPool2d(kernel_size=2, stride=2) on NHWC (upernet.py:48)."""
    if x.requires_grad and torch.is_grad_enabled():
        return _MaxPool2x2.apply(x)
    return ops.maxpool2x2s2(x)


# ------------------------------------------------------------------ resampling
class _Bilinear(Function):
    @staticmethod
    def forward(ctx, x, size):
        ctx.in_size = (x.shape[1], x.shape[2])
        return ops.bilinear(x, size)

    @staticmethod
    def backward(ctx, g):
        return ops.bilinear_bwd(g, ctx.in_size), None


def bilinear(x: Tensor, size) -> Tensor:
    """F.interpolate(mode='bilinear', align_corners=False) on NHWC."""
    size = (int(size[0]), int(size[1]))
    if size == (x.shape[1], x.shape[2]):
        return x
    return _Bilinear.apply(x, size)


class _UpsampleAdd(Function):
    """a + bilinear(b -> a's size)  (UperNet top-down path, upernet.py:127-135)."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.b_size = (b.shape[1], b.shape[2])
        if a.dim() == 4 and b.dim() == 4 and a.dtype == b.dtype:
            return ops.bilinear_add(a, b)          # one pass (bf16, factor 2 / 4), else copy + accumulate inside the library
        out = ops.copy_cast(a, out=torch.empty(a.shape, device=a.device, dtype=a.dtype))
        return ops.bilinear(b, (a.shape[1], a.shape[2]), out=out, accumulate=True)

    @staticmethod
    def backward(ctx, g):
        return g, ops.bilinear_bwd(g, ctx.b_size)


def upsample_add(a: Tensor, b: Tensor) -> Tensor:
    return _UpsampleAdd.apply(a, b)


class _ConvBNActUpsampleAddTrain(Function):
    """_ConvBNActTrain (statistics of one process) and _UpsampleAdd on its output as ONE node: ReLU(BN(conv(x))) + bilinear(b) --
    a UperNet lateral and the top-down add that is its only consumer (upernet.py:127-135).  The add kernel reads the lateral
    once anyway, so it forms BN + ReLU from the convolution output y on load (ops.bilinear_add_bn, bit-identical sum) and the
    normalised lateral is never written.  Backward: the gradient of the sum IS the gradient of the lateral's BatchNorm output
    (_UpsampleAdd passes it through), so the BatchNorm / convolution backward is _ConvBNActTrain's, plus the resize's for b."""

    @staticmethod
    def forward(ctx, x, weight, conv_bias, gamma, beta, running_mean, running_var, momentum, eps, pad, relu, b):
        cb = None if conv_bias is None else conv_bias.detach()
        y, stats_done = _cba_conv(x, weight, cb, pad, 0, False, running_mean, running_var, momentum)
        mean, var, _, p_local, _, _ = _bn_train_stats(y, weight.shape[0], running_mean, running_var, momentum, False, stats_done)
        out = ops.bilinear_add_bn(y, mean, var, gamma.detach(), beta.detach(), eps, relu, b)
        ctx.save_for_backward(x, weight, y, mean, var, gamma, beta)
        ctx.cfg = (pad, relu, eps, conv_bias is not None, p_local, (b.shape[1], b.shape[2]))
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, y, mean, var, gamma, beta = ctx.saved_tensors
        pad, relu, eps, has_bias, p_local, b_size = ctx.cfg
        db = ops.bilinear_bwd(g, b_size) if ctx.needs_input_grad[11] else None
        gout = g if g.dtype == y.dtype else to_compute(g, y.dtype)
        gm, bt = gamma.detach(), beta.detach()
        dgamma, dbeta = ops.bn_bwd_reduce(y, gout, mean, var, gm, bt, eps, relu)
        dbias = torch.zeros(weight.shape[0], device=x.device, dtype=torch.float32) if has_bias and ctx.needs_input_grad[2] else None
        dx, dw = _bn_bwd_and_grads(x, weight, y, gout, mean, var, gm, bt, eps, relu, dgamma, dbeta, p_local, pad, 0,
                                   ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dx, dw, dbias, dgamma, dbeta, None, None, None, None, None, None, db


def single_process_bn_train(norm: nn.Module) -> bool:
    """Train-mode BatchNorm whose batch statistics do not cross ranks."""
    return norm.training and _sync_world(_bn_sync_momentum(norm)[0]) == 1


def conv_bn_act_upsample_add(x: Tensor, conv: nn.Conv2d, norm: nn.Module, b: Tensor, *, relu: bool = True) -> Tensor:
    """upsample_add(conv_bn_act(x, conv, norm), b) for a ConvModule whose output has no other consumer.  bf16 training with the
    statistics of one process and a resize factor of 2 or 4: one node that never writes the normalised map
    (_ConvBNActUpsampleAddTrain, GDL_FUSE_BN_TAIL); everything else: the two separate nodes."""
    B, H, W = x.shape[0], x.shape[1], x.shape[2]
    n = conv.weight.shape[0]
    fused = (FUSE_BN_TAIL and single_process_bn_train(norm) and x.dtype == torch.bfloat16 and b.dtype == x.dtype and x.dim() == 4
             and b.dim() == 4 and b.is_contiguous() and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and b.shape[3] == n
             and not 0 < B * H * W <= ops.BN_SMALL_MAX_PIXELS      # (small maps: the one-launch BatchNorm of _ConvBNActTrain)
             and bool(ops._lib.load().gdl_bilinear_fwd_add_bn_ok(ops.BF16, B, b.shape[1], b.shape[2], H, W, n)))
    if not fused:
        return upsample_add(conv_bn_act(x, conv, norm, relu=relu), b)
    out = _ConvBNActUpsampleAddTrain.apply(x, conv.weight, conv.bias, norm.weight, norm.bias, norm.running_mean, norm.running_var,
                                           _bn_sync_momentum(norm)[1], norm.eps, conv.padding[0], relu, b)
    bump(norm.num_batches_tracked)
    return out


class _ConcatUpsample(Function):
    """cat([bilinear(x_i -> size) for x_i], channel dim) written straight into one NHWC buffer
    (upernet.py:103-109,144-152: no separate concat copy)."""

    @staticmethod
    def forward(ctx, size, *xs):
        b = xs[0].shape[0]
        chans = [x.shape[3] for x in xs]
        out = torch.empty((b, size[0], size[1], sum(chans)), device=xs[0].device, dtype=xs[0].dtype)
        off = 0
        for x, c in zip(xs, chans):
            ops.bilinear(x, size, out=out[..., off:off + c])
            off += c
        ctx.meta = [(x.shape[1], x.shape[2], x.shape[3]) for x in xs]
        return out

    @staticmethod
    def backward(ctx, g):
        grads, off = [], 0
        for i, (h, w, c) in enumerate(ctx.meta):
            if ctx.needs_input_grad[i + 1]:
                grads.append(ops.bilinear_bwd(g[..., off:off + c], (h, w)))
            else:
                grads.append(None)
            off += c
        return (None, *grads)


def concat_upsample(xs, size) -> Tensor:
    return _ConcatUpsample.apply((int(size[0]), int(size[1])), *xs)


class _AdaptivePool(Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.in_size = (x.shape[1], x.shape[2])
        return ops.adaptive_avgpool(x, s)

    @staticmethod
    def backward(ctx, g):
        return ops.adaptive_avgpool_bwd(g.contiguous(), ctx.in_size), None


def adaptive_avgpool(x: Tensor, s: int) -> Tensor:
    return _AdaptivePool.apply(x, s)


# ------------------------------------------------------------------ classifier tail
class _HeadLogits(Function):
    """1x1 conv to num_classes + bilinear to the input size -> NCHW f32 logits
    (segmentation_head.py:22-26 + dofa.py:89-96; fcn_head.py:69-84 with Dropout2d scale)."""

    @staticmethod
    def forward(ctx, feat, weight, bias, chan_scale, size):
        low = ops.head_1x1(feat, weight.detach(), None if bias is None else bias.detach(), chan_scale)
        ctx.save_for_backward(feat, weight, chan_scale)
        ctx.low_size = (feat.shape[1], feat.shape[2])
        ctx.has_bias = bias is not None
        return ops.upsample_logits(low, size)

    @staticmethod
    def backward(ctx, g):
        feat, weight, chan_scale = ctx.saved_tensors
        dlow = ops.upsample_logits_bwd(g.contiguous(), ctx.low_size)
        dfeat, dw, db = ops.head_1x1_bwd(feat, dlow, weight.detach(), chan_scale,
                                         need_dfeat=ctx.needs_input_grad[0])
        return dfeat, dw.view(weight.shape), (db if ctx.has_bias else None), None, None


class _Head1x1(Function):
    """The classifier alone: NHWC features -> [B, h, w, K] f32 logits at the feature resolution (the first half of _HeadLogits)."""

    @staticmethod
    def forward(ctx, feat, weight, bias, chan_scale):
        low = ops.head_1x1(feat, weight.detach(), None if bias is None else bias.detach(), chan_scale)
        ctx.save_for_backward(feat, weight, chan_scale)
        ctx.has_bias = bias is not None
        return low

    @staticmethod
    def backward(ctx, dlow):
        feat, weight, chan_scale = ctx.saved_tensors
        dfeat, dw, db = ops.head_1x1_bwd(feat, dlow.contiguous(), weight.detach(), chan_scale, need_dfeat=ctx.needs_input_grad[0])
        return dfeat, dw.view(weight.shape), (db if ctx.has_bias else None), None


class LowresLogits(NamedTuple):
    """Logits that have NOT been resized to the image yet: ``low`` [B, h, w, K] f32 (NHWC, as the 1x1 head writes them) and the
    ``size`` the reference's final ``F.interpolate(..., mode="bilinear")`` (dofa.py:89-105) would give them.  What a training
    step hands to ``gdlhip.nn.DiceLoss`` instead of the [B, K, H, W] tensor (round 5: the loss and its gradient are evaluated
    from ``low`` directly; the 168 MB of full-resolution logits per head are never written or read)."""

    low: Tensor
    size: tuple

    def materialise(self) -> Tensor:
        """The [B, K, H, W] f32 logits the reference's forward returns (differentiable)."""
        return _UpsampleLogits.apply(self.low, (int(self.size[0]), int(self.size[1])))


class _UpsampleLogits(Function):
    @staticmethod
    def forward(ctx, low, size):
        ctx.low_size = (low.shape[1], low.shape[2])
        return ops.upsample_logits(low, size)

    @staticmethod
    def backward(ctx, g):
        return ops.upsample_logits_bwd(g.contiguous(), ctx.low_size), None


FUSE_LOWRES_DICE = os.environ.get("GDL_LOWRES_DICE", "1") != "0"   # A/B switch: 0 = training steps materialise the full-resolution logits


def head_logits(feat: Tensor, conv: nn.Conv2d, size, chan_scale: Tensor | None = None, lowres: bool = False):
    """1x1 classifier + bilinear resize to ``size``: NCHW f32 logits; ``lowres``: the classifier's own map and the target size
    (LowresLogits) for a loss that does not need the resized tensor."""
    if lowres:
        return LowresLogits(_Head1x1.apply(feat, conv.weight, conv.bias, chan_scale), (int(size[0]), int(size[1])))
    return _HeadLogits.apply(feat, conv.weight, conv.bias, chan_scale, (int(size[0]), int(size[1])))


def logits_from_low(low: Tensor, size, lowres: bool = False):
    """What head_logits returns, from logits the head has already written at the feature resolution ([B, h, w, K] f32)."""
    if lowres:
        return LowresLogits(low, (int(size[0]), int(size[1])))
    return _UpsampleLogits.apply(low, (int(size[0]), int(size[1])))


# ------------------------------------------------------------------ losses
# The routes of the loss modules below: op stem (ops.<stem>_fwd / ops.<stem>_bwd) -> (number of state tensors the forward returns
# behind the loss and the backward takes again, what the route computes).  "low": bilinear(low -> size) of a head's NHWC map
# [B, h, w, K] (one-class: K = 1), forward and backward from that map; every backward recomputes from the saved logits.
# (SoftCrossEntropyLoss on a low-resolution map is the one route with a rule of its own: _SoftCELowres.)
_LOSS_ROUTES = {
    "dice_loss": (1, "smp DiceLoss / JaccardLoss / TverskyLoss (multiclass) on NCHW logits; state: the per-class sums"),
    "dice_loss_lowres": (1, "the same losses, low"),
    "dice_binary_loss": (1, "smp DiceLoss / JaccardLoss / TverskyLoss (binary): one logit per target entry"),
    "dice_binary_lowres": (1, "the same losses, one-class low"),
    "soft_ce": (0, "smp SoftCrossEntropyLoss on NCHW logits"),
    "cross_entropy": (1, "torch CrossEntropyLoss on NCHW logits; state: the divisor the forward left on the device"),
    "cross_entropy_lowres": (1, "torch CrossEntropyLoss, low"),
    "focal": (1, "smp FocalLoss (multiclass) on NCHW logits; state: the divisor the forward left on the device"),
    "focal_binary": (1, "smp FocalLoss (binary): one logit per target entry, positive where the target is 1"),
    "focal_lowres": (1, "smp FocalLoss (multiclass), low"),
    "focal_binary_lowres": (1, "smp FocalLoss (binary), one-class low"),
    "soft_bce": (0, "smp SoftBCEWithLogitsLoss on NCHW logits and an int64 or f32 target of the same numel"),
    "soft_bce_lowres": (0, "smp SoftBCEWithLogitsLoss, one-class low"),
    "lovasz": (2, "smp LovaszLoss (multiclass) on NCHW logits; state: the Jaccard coefficients in pixel order, the segments' weights"),
    "lovasz_binary": (2, "smp LovaszLoss (binary): one logit per target entry, positive where the target is 1"),
}


class _Loss(Function):
    """The autograd node of every route in _LOSS_ROUTES: ``ops.<stem>_fwd(x, target[, size][, eps], options=)`` returns the loss
    and the route's state tensors; ``ops.<stem>_bwd(x, target[, size], *state, g, 1.0[, eps], options=)`` is d loss / d x.
    ``size`` (the low-resolution routes) and ``eps`` (the Dice family) are None where the ops do not take them."""

    @staticmethod
    def forward(ctx, stem, x, target, options, size, eps):
        out = getattr(ops, stem + "_fwd")(x, target, *(a for a in (size, eps) if a is not None), options=options)
        loss, *state = out if _LOSS_ROUTES[stem][0] else (out,)
        ctx.save_for_backward(x, target, *state)
        ctx.stem, ctx.options, ctx.size, ctx.eps = stem, options, size, eps
        return loss

    @staticmethod
    def backward(ctx, g):
        x, target, *state = ctx.saved_tensors
        size, eps = (() if a is None else (a,) for a in (ctx.size, ctx.eps))
        dx = getattr(ops, ctx.stem + "_bwd")(x, target, *size, *state, g.contiguous().float(), 1.0, *eps, options=ctx.options)
        return None, dx, None, None, None, None


def _binary_lowres_ok(low: Tensor, size, yt: Tensor) -> bool:
    """A one-class head's map that the binary low-resolution kernels take in place of the resized logits -- where that is the
    faster route (ops.binary_lowres_pays: the measured factors; a larger one materialises, as every other excluded case)."""
    return (FUSE_LOWRES_DICE and low.dim() == 4 and low.shape[3] == 1 and low.dtype == torch.float32 and ops.binary_lowres_pays(low, size)
            and yt.dim() == 3 and tuple(yt.shape[1:]) == size)


def _loss_input(y_pred, y_true: Tensor, lowres: str | None, squeeze: bool):
    """The start of every loss's forward: ``(x, target, size)``.  ``lowres``: the low-resolution kernels the loss has for this
    call, "multiclass" ([B, h, w, K] maps), "binary" (the one-class head's [B, h, w, 1]) or None.  Where ``y_pred`` is a
    LowresLogits those kernels take, ``x`` is its contiguous map, ``target`` the [B, H, W] view of ``y_true`` and ``size`` the
    image size.  Everything else gets ``size`` None and ``x`` the contiguous f32 logits (a LowresLogits materialised), with an
    un-squeezed [B, 1, H, W] ``y_true`` viewed as [B, H, W] if ``squeeze`` (smp views the target as [B, -1]: the same)."""
    if isinstance(y_pred, LowresLogits):
        # a training step's not-yet-resized logits: the loss (and its gradient) straight from the low-resolution map
        low, size = y_pred.low, (int(y_pred.size[0]), int(y_pred.size[1]))
        yt = y_true[:, 0] if y_true.dim() == 4 and y_true.shape[1] == 1 else y_true
        if lowres == "multiclass":
            ok = FUSE_LOWRES_DICE and ops.dice_lowres_ok(low, size) and low.dtype == torch.float32 and tuple(yt.shape[1:]) == size
        else:
            ok = lowres == "binary" and _binary_lowres_ok(low, size, yt) and low.shape[0] == yt.shape[0]
        if ok:
            return low.contiguous(), yt, size
        y_pred = y_pred.materialise()
    if y_pred.dtype != torch.float32 or not y_pred.is_contiguous():
        y_pred = y_pred.float().contiguous()
    if squeeze and y_true.dim() == y_pred.dim() >= 2 and y_true.shape[1] == 1:
        y_true = y_true[:, 0]
    return y_pred, y_true, None


def _checked_ignore_index(name: str, ignore_index):
    """``ignore_index`` as an int, or None (no pixel is ignored)."""
    if ignore_index is None:
        return None
    if isinstance(ignore_index, bool) or int(ignore_index) != ignore_index or not -2**63 <= int(ignore_index) < 2**63:
        raise ValueError(f"{name}: ignore_index must be an int64 value or None (got {ignore_index!r})")
    return int(ignore_index)


def _check_mode(name: str, mode, unimplemented: tuple | None = ("multilabel",)) -> None:
    """A mode smp has and gdlhip does not (``unimplemented``; None: any other) is a NotImplementedError, an unknown one a
    ValueError."""
    if mode not in ("multiclass", "binary"):
        if unimplemented is None or mode in unimplemented:
            raise NotImplementedError(f"gdlhip {name} implements mode='multiclass' and mode='binary' (got {mode!r})")
        raise ValueError(f"{name}: unknown mode {mode!r}")


def _check_reduction(name: str, reduction, unimplemented: tuple = ("none",)) -> None:
    """As _check_mode, for ``reduction``."""
    if reduction not in ("mean", "sum"):
        if reduction in unimplemented:
            raise NotImplementedError(f"gdlhip {name} implements reduction='mean' and 'sum' (got {reduction!r})")
        raise ValueError(f"{name}: unknown reduction {reduction!r}")


class _DiceFamily(nn.Module):
    """What DiceLoss, JaccardLoss and TverskyLoss share: the checks of smp's common constructor arguments and the forward that
    picks the full-resolution, low-resolution (LowresLogits) or binary kernels.  A subclass sets ``mode``, ``eps``, ``classes``
    and ``options`` (which selects the loss)."""

    def _check_common(self, mode, classes, from_logits, ignore_index, **floats):
        """The validated (classes, ignore_index); ``floats``: named values that must be finite."""
        name = type(self).__name__
        _check_mode(name, mode, None)
        if not from_logits:
            raise NotImplementedError(f"gdlhip {name} takes logits (from_logits=True); from_logits=False is not implemented")
        if classes is not None:
            classes = tuple(int(c) for c in classes)
            if len(classes) == 0 or len(set(classes)) != len(classes) or min(classes) < 0:
                raise ValueError(f"{name}: classes must be a non-empty list of distinct class indices >= 0 (got {classes})")
            if mode == "binary" and classes != (0,):
                raise ValueError(f"{name}(binary) has the single class 0: classes must be None or [0] (got {list(classes)})")
        ignore_index = _checked_ignore_index(name, ignore_index)
        for key, v in floats.items():
            if not math.isfinite(v):
                raise ValueError(f"{name}: {key} must be finite (got {v})")
        return classes, ignore_index

    def _check_classes(self, K: int) -> None:
        if self.classes is not None and max(self.classes) >= K:
            raise ValueError(f"{type(self).__name__}: classes {list(self.classes)} out of range for {K} classes")

    def forward(self, y_pred, y_true: Tensor) -> Tensor:
        binary = self.mode == "binary"
        x, y_true, size = _loss_input(y_pred, y_true, self.mode, squeeze=not binary)
        if not binary:
            self._check_classes(x.shape[1 if size is None else 3])
        elif size is None and (x.shape[0] != y_true.shape[0] or x.numel() != y_true.numel()):
            msg = f"{type(self).__name__}(binary): y_pred {tuple(x.shape)} and y_true {tuple(y_true.shape)} do not match"
            raise ValueError(msg)
        if binary:
            stem = "dice_binary_loss" if size is None else "dice_binary_lowres"
        else:
            stem = "dice_loss" if size is None else "dice_loss_lowres"
        return _Loss.apply(stem, x, y_true.long().contiguous(), self.options, size, self.eps)


class DiceLoss(_DiceFamily):
    """Drop-in for ``segmentation_models_pytorch.losses.DiceLoss`` (smp 0.5.0 losses/dice.py) in the two modes the reference's
    configs use: ``mode="multiclass"`` (configs/dofa_config_RGB.yaml:58-61, segformer) and ``mode="binary"``
    (configs/unetplus_config_RGB.yaml, ``num_classes: 1``), with smp's constructor options evaluated inside the HIP kernels:

    - ``ignore_index`` (any int, e.g. 255 or -1): pixels whose target equals it are left out of every sum and get a zero gradient;
    - ``smooth``: ``score_k = (2 I_k + smooth) / max(P_k + Y_k + smooth, eps)``;
    - ``log_loss``: ``-log(max(score_k, eps))`` instead of ``1 - score_k``;
    - ``classes``: the mean runs over the listed classes only (distinct indices in ``0..K-1``, checked at the first forward, when
      ``K`` is known; binary mode takes ``None`` or ``[0]``).

    A class without a valid (not ignored) pixel in the batch contributes 0.  A target value outside ``0..K-1`` that is not
    ``ignore_index`` matches no class while its probabilities still count in the denominators (unchanged behaviour).  With every
    option at its default the plain kernels run and the results are bit-identical to earlier builds.  ``from_logits=False`` is
    not implemented and raises.

    ``y_pred`` may be ``LowresLogits`` (f32, ``GDL_LOWRES_DICE`` on): multiclass with K <= 16 and an upsample by at most 64 per
    direction, or binary with the one-class head's ``[B, h, w, 1]`` map and an upsample by at most
    ``ops.BINARY_LOWRES_MAX_FACTOR`` = 8 per direction (the kernels take factors up to 64, but beyond 8 materialising was measured
    to be faster: ``ops.binary_lowres_pays``); the loss and d(low) then come from that map and the resized logits are never
    written.  Other cases materialise them."""

    def __init__(self, mode: str = "multiclass", classes=None, log_loss: bool = False, from_logits: bool = True,
                 smooth: float = 0.0, ignore_index=None, eps: float = 1e-7) -> None:
        super().__init__()
        smooth = float(smooth)
        classes, ignore_index = self._check_common(mode, classes, from_logits, ignore_index, smooth=smooth)
        self.mode, self.eps = mode, eps
        self.classes, self.log_loss, self.smooth, self.ignore_index = classes, bool(log_loss), smooth, ignore_index
        # None = smp's defaults: the plain entry points
        self.options = None
        if classes is not None or self.log_loss or smooth != 0.0 or ignore_index is not None:
            self.options = ops.DiceOptions(ignore_index, smooth, self.log_loss, classes)


class JaccardLoss(_DiceFamily):
    """Stand-in for ``segmentation_models_pytorch.losses.JaccardLoss`` (smp 0.5.0 constructor signature and defaults) in modes
    ``"multiclass"`` and ``"binary"``, evaluated by the gdl_overlap_* HIP entry points on the per-class sums the Dice kernels
    reduce.  smp is not installed where this was written, so parity with smp itself is unpinned; the formula is:

    with ``p`` = softmax (binary: sigmoid) of the logits, ``I_k = sum p_k [y=k]``, ``P_k = sum p_k``, ``Y_k = count(y=k)`` over
    batch and pixels, ``score_k = (I_k + smooth) / max(P_k + Y_k - I_k + smooth, eps)``; the per-class loss is ``1 - score_k``, or
    ``-log(max(score_k, eps))`` with ``log_loss``; a class with ``Y_k = 0`` contributes 0; the result is the mean over ``classes``
    (all K when None; absent classes still count in the divisor).  There is no ``ignore_index``, as in smp.

    Targets are ``[B,H,W]`` or ``[B,1,H,W]``.  ``y_pred`` may be ``LowresLogits``: the loss and d(low) come from the head's own
    map under DiceLoss's conditions (f32; multiclass: K <= 16 and factor <= 64, binary: K = 1 and factor <= 8); other cases
    materialise the logits.  ``mode="multilabel"`` and ``from_logits=False`` raise ``NotImplementedError``."""

    def __init__(self, mode: str = "multiclass", classes=None, log_loss: bool = False, from_logits: bool = True,
                 smooth: float = 0.0, eps: float = 1e-7) -> None:
        super().__init__()
        smooth = float(smooth)
        classes, _ = self._check_common(mode, classes, from_logits, None, smooth=smooth)
        self.mode, self.eps = mode, eps
        self.classes, self.log_loss, self.smooth = classes, bool(log_loss), smooth
        self.options = ops.OverlapOptions("jaccard", None, smooth, self.log_loss, classes)


class TverskyLoss(_DiceFamily):
    """Stand-in for ``segmentation_models_pytorch.losses.TverskyLoss`` (smp 0.5.0 constructor signature and defaults), focal form
    included, in modes ``"multiclass"`` and ``"binary"``, evaluated by the gdl_overlap_* HIP entry points.  smp is not installed
    where this was written, so parity with smp itself is unpinned; the formula is:

    with ``I_k``, ``P_k``, ``Y_k`` as in JaccardLoss, taken over the pixels whose target is not ``ignore_index``,
    ``score_k = (I_k + smooth) / max(I_k + alpha (P_k - I_k) + beta (Y_k - I_k) + smooth, eps)`` (``alpha`` weighs false
    positives, ``beta`` false negatives; ``alpha = beta = 0.5`` is Dice, ``alpha = beta = 1`` Jaccard); per-class loss, ``Y_k = 0``
    rule and the mean ``m`` over ``classes`` as in JaccardLoss; the result is ``m ** gamma``.  Its gradient carries the factor
    ``gamma * m ** (gamma - 1)``, which is DEFINED AS 0 WHEN ``m <= 0`` and ``gamma != 1`` (torch would give inf or nan there for
    ``gamma < 1``: a perfect prediction gets a zero gradient, not a non-finite one), and the result itself is 0 there.
    An ignored pixel gets an exactly zero gradient in every class.  ``alpha, beta >= 0`` and ``gamma > 0`` are required.

    Targets, ``LowresLogits`` and the unimplemented arguments: as JaccardLoss."""

    def __init__(self, mode: str = "multiclass", classes=None, log_loss: bool = False, from_logits: bool = True,
                 smooth: float = 0.0, ignore_index=None, eps: float = 1e-7, alpha: float = 0.5, beta: float = 0.5,
                 gamma: float = 1.0) -> None:
        super().__init__()
        smooth, alpha, beta, gamma = float(smooth), float(alpha), float(beta), float(gamma)
        classes, ignore_index = self._check_common(mode, classes, from_logits, ignore_index, smooth=smooth, alpha=alpha,
                                                   beta=beta, gamma=gamma)
        if alpha < 0.0 or beta < 0.0 or gamma <= 0.0:
            raise ValueError(f"TverskyLoss: alpha, beta >= 0 and gamma > 0 are required (got {alpha}, {beta}, {gamma})")
        self.mode, self.eps = mode, eps
        self.classes, self.log_loss, self.smooth, self.ignore_index = classes, bool(log_loss), smooth, ignore_index
        self.alpha, self.beta, self.gamma = alpha, beta, gamma
        self.options = ops.OverlapOptions("tversky", ignore_index, smooth, self.log_loss, classes, alpha, beta, gamma)


class _SoftCELowres(Function):
    """smp SoftCrossEntropyLoss of bilinear(low -> size) from the low-resolution map.  ``fused``: the forward also leaves the
    unscaled patches of d(low) behind and the backward only reduces them (ops.soft_ce_lowres_fwd)."""

    @staticmethod
    def forward(ctx, low, target, size, options, fused):
        loss, state = ops.soft_ce_lowres_fwd(low, target, size, options, fused=fused and ctx.needs_input_grad[0])
        ctx.save_for_backward(low, target, state)
        ctx.size, ctx.options = size, options
        return loss

    @staticmethod
    def backward(ctx, g):
        low, target, state = ctx.saved_tensors
        dlow = ops.soft_ce_lowres_bwd(low, target, ctx.size, g.contiguous().float(), 1.0, ctx.options, state=state)
        return dlow, None, None, None, None


# The low-resolution backward form: 1 = the forward emits the patches of d(low) (one softmax evaluation per pixel and step), 0 = the
# backward recomputes them.  The default is the faster of the two at batch 64, K = 5, both DOFA heads.
SOFT_CE_LOWRES_FUSED = os.environ.get("GDL_SOFT_CE_FUSED", "1") != "0"


class SoftCrossEntropyLoss(nn.Module):
    """Drop-in for ``segmentation_models_pytorch.losses.SoftCrossEntropyLoss`` (smp 0.5.0 losses/soft_ce.py and
    ``label_smoothed_nll_loss`` in losses/_functional.py), the loss of the reference's quick-start notebook
    (notebooks/00_quickstart.ipynb: ``SoftCrossEntropyLoss(smooth_factor=0.1)``), evaluated by the gdl_soft_ce_* HIP kernels.
    smp is not installed where this was written, so parity with smp itself is unpinned: the formula below is restated from its
    source and tested against ``F.cross_entropy(..., label_smoothing=e, reduction="sum") / N``, which it equals.

    With ``e = smooth_factor`` (None = 0), ``K`` classes and ``N = B*H*W`` (every pixel, ignored ones included), per valid pixel
    ``L_i = logsumexp_k x_ik - (1 - e) x_{i,y_i} - (e / K) sum_k x_ik``; ``reduction="mean"`` is ``sum_i L_i / N`` -- the divisor is
    N, not the valid count (smp zero-fills the masked entries and calls ``.mean()``; ``torch.nn.CrossEntropyLoss`` divides by the
    valid count) -- and ``reduction="sum"`` is ``sum_i L_i``.  A pixel whose target equals ``ignore_index`` (compared as int64;
    ``None``: no pixel) adds nothing and gets an exactly zero gradient.  A target outside ``0..K-1`` that is not ``ignore_index``
    would trip a device assert in smp's ``gather``; here it is treated as ignored.  ``reduction="none"`` and ``dim != 1`` raise
    ``NotImplementedError``.  Targets are ``[B,H,W]`` or ``[B,1,H,W]``.

    ``y_pred`` may be ``LowresLogits`` (a DOFA training / validation step): the loss and d(low) come straight from the head's own
    map, the [B, K, H, W] tensor is never written (K <= 16, factor <= 64 as for DiceLoss; other shapes materialise)."""

    def __init__(self, reduction: str = "mean", smooth_factor: float | None = None, ignore_index: int | None = -100,
                 dim: int = 1) -> None:
        super().__init__()
        _check_reduction("SoftCrossEntropyLoss", reduction)
        if dim != 1:
            raise NotImplementedError(f"gdlhip SoftCrossEntropyLoss takes the class dimension at dim=1 (got dim={dim})")
        eps = 0.0 if smooth_factor is None else float(smooth_factor)
        if not math.isfinite(eps) or not 0.0 <= eps <= 1.0:
            raise ValueError(f"SoftCrossEntropyLoss: smooth_factor must be a finite value in [0, 1] (got {smooth_factor!r})")
        ignore_index = _checked_ignore_index("SoftCrossEntropyLoss", ignore_index)
        self.reduction, self.smooth_factor, self.ignore_index, self.dim = reduction, smooth_factor, ignore_index, dim
        self.options = ops.SoftCEOptions(eps, ignore_index, reduction == "mean")

    def forward(self, y_pred, y_true: Tensor) -> Tensor:
        x, y_true, size = _loss_input(y_pred, y_true, "multiclass", squeeze=True)
        if size is not None:
            return _SoftCELowres.apply(x, y_true.long().contiguous(), size, self.options, SOFT_CE_LOWRES_FUSED)
        if x.dim() != 4:
            raise ValueError(f"SoftCrossEntropyLoss: [B, K, H, W] logits expected (got {tuple(x.shape)})")
        return _Loss.apply("soft_ce", x, y_true.long().contiguous(), self.options, None, None)


class CrossEntropyLoss(nn.Module):
    """``torch.nn.CrossEntropyLoss`` (argument names, order and defaults) for class-index targets, evaluated by the
    gdl_cross_entropy_* HIP kernels; the reference of every number is ``F.cross_entropy`` itself.

    With ``e = label_smoothing``, ``K`` classes, ``w_k = weight[k]`` (all 1 without ``weight``), ``W = sum_k w_k`` and
    ``lse_i = logsumexp_k x_ik``, per valid pixel
    ``L_i = (1 - e) w_{y_i} (lse_i - x_{i,y_i}) + (e / K) sum_k w_k (lse_i - x_ik)``; ``reduction="mean"`` is
    ``sum_i L_i / D`` with ``D = sum_i w_{y_i}`` over the valid pixels, ``reduction="sum"`` is ``sum_i L_i``.  A pixel whose target
    equals ``ignore_index`` (compared as int64) adds nothing and gets an exactly zero gradient.  A zero-weight class adds nothing
    to ``D`` or to the first term; its pixels still carry the smoothing term, as in torch.  ``weight`` is a buffer under torch's
    name (the same state-dict key), held as f32; the kernels read it through its device pointer at call time and ``D`` is formed
    and applied on the device, so nothing is copied to the host in forward or backward.  Targets are int64 ``[B,H,W]`` or
    ``[B,1,H,W]``.

    Two deliberate deviations from torch:

    1. A target outside ``0..K-1`` that is not ``ignore_index`` is treated as ignored (torch device-asserts on it): the target is
       only ever compared, never used as an index -- the rule of ``SoftCrossEntropyLoss``.
    2. With ``reduction="mean"`` and ``D == 0`` (every pixel ignored, or every valid pixel of a zero-weight class) the loss is 0
       and every gradient is 0, where torch returns NaN: a NaN would poison the weights inside a captured step that cannot look
       at it.  ``FocalLoss`` does the same.

    ``reduction="none"``, class-probability (floating point) targets and a non-``None`` ``size_average`` / ``reduce`` raise
    ``NotImplementedError``.

    ``y_pred`` may be ``LowresLogits`` (a DOFA training / validation step): the loss and d(low) come straight from the head's own
    map, the [B, K, H, W] tensor is never written (K <= 16, factor <= 64 as for SoftCrossEntropyLoss; other shapes materialise)."""

    def __init__(self, weight: Tensor | None = None, size_average=None, ignore_index: int | None = -100, reduce=None,
                 reduction: str = "mean", label_smoothing: float = 0.0) -> None:
        super().__init__()
        if size_average is not None or reduce is not None:
            raise NotImplementedError("gdlhip CrossEntropyLoss implements reduction= only (size_average and reduce must be None)")
        _check_reduction("CrossEntropyLoss", reduction)
        label_smoothing = float(label_smoothing)
        if not 0.0 <= label_smoothing <= 1.0:      # (NaN and the infinities fail the comparison)
            raise ValueError(f"CrossEntropyLoss: label_smoothing must be a finite value in [0, 1] (got {label_smoothing})")
        ignore_index = _checked_ignore_index("CrossEntropyLoss", ignore_index)      # (None, which torch does not take: no pixel is ignored)
        if weight is not None:
            if not isinstance(weight, Tensor):      # a yaml config spells the weights as a list
                weight = torch.as_tensor(weight, dtype=torch.float32)
            if weight.dim() != 1 or weight.numel() < 1:
                raise ValueError(f"CrossEntropyLoss: weight must be 1-D, one value per class (got shape {tuple(weight.shape)})")
            weight = weight.detach().float().contiguous()
            if not bool((torch.isfinite(weight) & (weight >= 0)).all()):
                raise ValueError("CrossEntropyLoss: every weight must be finite and >= 0")
        self.ignore_index, self.reduction, self.label_smoothing = ignore_index, reduction, label_smoothing
        self.register_buffer("weight", weight)

    def _options(self, K: int) -> ops.CrossEntropyOptions:
        """The options with the buffer as it is now (a ``.to(device)`` moves it): f32 and contiguous, which it already is unless a
        state dict or a cast changed it."""
        w = self.weight
        if w is not None:
            if w.dim() != 1 or w.numel() != K:
                raise ValueError(f"CrossEntropyLoss: weight holds {tuple(w.shape)} values for {K} classes")
            w = w.detach().float().contiguous()
        return ops.CrossEntropyOptions(self.label_smoothing, self.ignore_index, self.reduction == "mean", w)

    def forward(self, y_pred, y_true: Tensor) -> Tensor:
        if y_true.is_floating_point() or y_true.is_complex():
            raise NotImplementedError("gdlhip CrossEntropyLoss implements class-index targets only (got class probabilities)")
        x, y_true, size = _loss_input(y_pred, y_true, "multiclass", squeeze=True)
        if size is None and x.dim() != 4:
            raise ValueError(f"CrossEntropyLoss: [B, K, H, W] logits expected (got {tuple(x.shape)})")
        stem, K = ("cross_entropy", x.shape[1]) if size is None else ("cross_entropy_lowres", x.shape[3])
        return _Loss.apply(stem, x, y_true.long().contiguous(), self._options(K), size, None)


class FocalLoss(nn.Module):
    """Stand-in for ``segmentation_models_pytorch.losses.FocalLoss`` (smp 0.5.0 constructor signature and defaults; losses/focal.py
    and ``focal_loss_with_logits`` in losses/_functional.py) in modes ``"multiclass"`` and ``"binary"``, evaluated by the
    gdl_focal_* HIP kernels.  smp is not installed where this was written, so parity with smp itself is unpinned; the formula is:

    per element, for logit ``x`` and ``z`` in {0, 1}: ``s = (2z - 1) x``, ``L = softplus(-s)`` (BCE with logits, ``-log pt``),
    ``q = sigmoid(-s) = 1 - pt``, ``f = q ** gamma`` -- with ``reduced_threshold = th``: ``f = (q / th) ** gamma``, and ``f = 1``
    where ``pt < th`` --, ``a = alpha z + (1 - alpha)(1 - z)`` (1 when ``alpha`` is None); the element's loss is ``a f L``.
    Multiclass (logits ``[B,K,H,W]``, target ``[B,H,W]`` or ``[B,1,H,W]``): ``z = [y == k]`` for every class k.  Binary (logits
    and target of equal numel and batch size): ``z = [y == 1]``; ANY OTHER target value that is not ``ignore_index`` counts as 0.
    A pixel is valid unless ``y == ignore_index`` (compared as int64).  The loss is the sum over classes and valid pixels, divided
    by the number of valid pixels for ``reduction="mean"`` (smp: the mean per class over the not-ignored pixels, classes added)
    and as it is for ``"sum"``.

    - The gradient is DEFINED by the closed form ``-(2z - 1) a f (gamma pt L + q)`` (``-(2z - 1) a q`` on the ``f = 1`` branch):
      finite for every ``gamma >= 0``, where torch's autograd of ``q ** gamma`` gives NaN at ``q = 0`` for ``0 < gamma < 1``.
    - Without a valid pixel the loss is 0 and the gradient exactly 0 (smp's mean of an empty tensor is NaN).
    - An ignored pixel gets an exactly zero gradient in every class.
    - A multiclass target outside ``0..K-1`` that is not ``ignore_index`` matches no class and stays a valid all-negative pixel,
      as in smp; the target is never used as an index.

    ``y_pred`` may be ``LowresLogits``: the loss and d(low) come from the head's own map under DiceLoss's conditions (f32;
    multiclass: K <= 16 and factor <= 64, binary: K = 1 and factor <= ``ops.BINARY_LOWRES_MAX_FACTOR`` = 8, beyond which
    materialising was measured to be faster); other cases materialise the logits.  ``normalized=True``, ``reduction="none"`` /
    ``"batchwise_mean"`` and ``mode="multilabel"`` raise ``NotImplementedError``."""

    def __init__(self, mode: str, alpha: float | None = None, gamma: float | None = 2.0, ignore_index: int | None = None,
                 reduction: str | None = "mean", normalized: bool = False, reduced_threshold: float | None = None) -> None:
        super().__init__()
        _check_mode("FocalLoss", mode)
        if normalized:
            raise NotImplementedError("gdlhip FocalLoss implements normalized=False only")
        _check_reduction("FocalLoss", reduction, ("none", "batchwise_mean"))
        gamma = float(gamma)
        if not math.isfinite(gamma) or gamma < 0.0:
            raise ValueError(f"FocalLoss: gamma must be finite and >= 0 (got {gamma})")
        if alpha is not None:
            alpha = float(alpha)
            if not 0.0 <= alpha <= 1.0:
                raise ValueError(f"FocalLoss: alpha must be None or in [0, 1] (got {alpha})")
        if reduced_threshold is not None:
            reduced_threshold = float(reduced_threshold)
            if not 0.0 < reduced_threshold <= 1.0:
                raise ValueError(f"FocalLoss: reduced_threshold must be None or in (0, 1] (got {reduced_threshold})")
        ignore_index = _checked_ignore_index("FocalLoss", ignore_index)
        self.mode, self.alpha, self.gamma, self.ignore_index = mode, alpha, gamma, ignore_index
        self.reduction, self.normalized, self.reduced_threshold = reduction, False, reduced_threshold
        self.options = ops.FocalOptions(gamma, alpha, ignore_index, reduction == "mean", reduced_threshold)

    def forward(self, y_pred, y_true: Tensor) -> Tensor:
        binary = self.mode == "binary"
        x, y_true, size = _loss_input(y_pred, y_true, self.mode, squeeze=not binary)
        if size is None:
            if binary and (x.shape[0] != y_true.shape[0] or x.numel() != y_true.numel()):
                raise ValueError(f"FocalLoss(binary): y_pred {tuple(x.shape)} and y_true {tuple(y_true.shape)} do not match")
            if not binary and x.dim() != 4:
                raise ValueError(f"FocalLoss(multiclass): [B, K, H, W] logits expected (got {tuple(x.shape)})")
        stem = ("focal_binary" if binary else "focal") + ("" if size is None else "_lowres")
        return _Loss.apply(stem, x, y_true.long().contiguous(), self.options, size, None)


class SoftBCEWithLogitsLoss(nn.Module):
    """Stand-in for ``segmentation_models_pytorch.losses.SoftBCEWithLogitsLoss`` (smp 0.5.0 constructor signature and defaults;
    losses/soft_bce.py), evaluated by the gdl_soft_bce_* HIP kernels.  smp is not installed where this was written, so parity with
    smp unpinned; the formula is:

    per element, for logit ``x``, raw target value ``y``, ``w`` / ``p`` the ``weight`` / ``pos_weight`` of the element's channel
    (1 when absent): ``t = (1 - y) smooth_factor + y (1 - smooth_factor)`` (``y`` when ``smooth_factor`` is None),
    ``l = w ((1 - t) x + (1 + (p - 1) t) softplus(-x))`` -- ``F.binary_cross_entropy_with_logits(x, t, w, pos_weight=p)`` -- and
    ``dl/dx = w ((1 - t) - (1 + (p - 1) t) sigmoid(-x))``.  The loss is the sum of ``l`` over the elements with
    ``y != ignore_index``, for ``reduction="mean"`` divided by the number of ALL elements, ignored ones included (smp's
    ``loss.mean()``; FocalLoss divides by the valid count instead), and as it is for ``"sum"``.

    - The ignore test is on the raw target, before smoothing: an integer target compares as int64, a floating one as floating
      point (torch's ``y_true != ignore_index``).
    - Targets are values, not labels: any fractional ``y_true`` is legal.  int64 and f32 targets go to the kernels as they are;
      other integer dtypes are converted to int64, other floating dtypes to f32.
    - An ignored element contributes exactly 0 and gets an exactly zero gradient: a select, not a multiplication, so a non-finite
      logit under an ignored pixel does not poison the sum.
    - ``y_true`` may have any shape with ``y_pred``'s batch size and numel (``[B,H,W]`` against ``[B,1,H,W]`` logits, as
      ``FocalLoss(mode="binary")`` accepts; torch itself would raise).
    - ``weight`` and ``pos_weight`` are buffers under smp's names (the same state-dict keys): None, a tensor of numel 1, or a tensor
      that varies only over the channel dimension of ``[B,C,H,W]`` logits, shape ``[C,1,1]`` or ``[1,C,1,1]``; any other shape raises
      ``NotImplementedError``.  The kernels read them through device pointers at call time; nothing is copied to the host.
    - ``reduction="none"`` raises ``NotImplementedError``.

    ``y_pred`` may be ``LowresLogits``: for a one-class head's f32 map with a factor <= ``ops.BINARY_LOWRES_MAX_FACTOR`` = 8 the
    loss and d(low) come from the map itself (the routing of ``FocalLoss(mode="binary")``); other cases materialise the logits."""

    def __init__(self, weight: Tensor | None = None, ignore_index: int | None = -100, reduction: str = "mean",
                 smooth_factor: float | None = None, pos_weight: Tensor | None = None) -> None:
        super().__init__()
        _check_reduction("SoftBCEWithLogitsLoss", reduction)
        if smooth_factor is not None:
            smooth_factor = float(smooth_factor)
            if not 0.0 <= smooth_factor <= 1.0:      # (NaN and the infinities fail the comparison)
                raise ValueError(f"SoftBCEWithLogitsLoss: smooth_factor must be None or in [0, 1] (got {smooth_factor})")
        ignore_index = _checked_ignore_index("SoftBCEWithLogitsLoss", ignore_index)
        for name, t in (("weight", weight), ("pos_weight", pos_weight)):
            if t is None:
                continue
            if not isinstance(t, Tensor):
                raise TypeError(f"SoftBCEWithLogitsLoss: {name} must be a Tensor or None (got {type(t).__name__})")
            shape = tuple(t.shape)
            per_channel = (len(shape) == 3 and shape[1:] == (1, 1)) or (len(shape) == 4 and shape[0] == 1 and shape[2:] == (1, 1))
            if t.numel() != 1 and not per_channel:
                raise NotImplementedError(f"gdlhip SoftBCEWithLogitsLoss implements a {name} of one value or one per channel, "
                                          f"shape [C,1,1] or [1,C,1,1] (got {shape})")
        self.ignore_index, self.reduction, self.smooth_factor = ignore_index, reduction, smooth_factor
        self.register_buffer("weight", weight)
        self.register_buffer("pos_weight", pos_weight)

    def _options(self) -> ops.SoftBCEOptions:
        """The options with the buffers as they are now (a ``.to(device)`` moves them): f32 and contiguous, which they already are
        unless they were registered otherwise."""
        w, p = (None if t is None else t.detach().float().contiguous() for t in (self.weight, self.pos_weight))
        return ops.SoftBCEOptions(self.smooth_factor, self.ignore_index, self.reduction == "mean", w, p)

    @staticmethod
    def _target(y_true: Tensor) -> Tensor:
        if y_true.dtype not in (torch.int64, torch.float32):
            y_true = y_true.float() if y_true.is_floating_point() else y_true.long()
        return y_true.contiguous()

    def forward(self, y_pred, y_true: Tensor) -> Tensor:
        x, y_true, size = _loss_input(y_pred, y_true, "binary", squeeze=False)
        if size is not None:
            return _Loss.apply("soft_bce_lowres", x, self._target(y_true), self._options(), size, None)
        if x.dim() < 1 or x.shape[0] != y_true.shape[0] or x.numel() != y_true.numel():
            raise ValueError(f"SoftBCEWithLogitsLoss: y_pred {tuple(x.shape)} and y_true {tuple(y_true.shape)} do not match")
        if x.dim() != 4:      # no channel dimension to speak of: one "channel" of everything behind the batch
            x = x.reshape(x.shape[0], 1, 1, -1)
        return _Loss.apply("soft_bce", x, self._target(y_true), self._options(), None, None)


class LovaszLoss(nn.Module):
    """Stand-in for ``segmentation_models_pytorch.losses.LovaszLoss`` (smp 0.5.0 constructor signature and defaults; losses/lovasz.py)
    in modes ``"multiclass"`` and ``"binary"``, evaluated by the gdl_lovasz_* HIP kernels on the library's own segmented radix sort.
    smp is not installed where this was written, so parity with smp itself is unpinned; the definition is:

    **Jaccard coefficients.**  A segment of n errors is sorted descending, ties by ascending flat index
    (``torch.sort(descending=True, stable=True)``).  At rank r (0-based), with the label bit ``z_r``, ``G = sum z``,
    ``P_r = sum_{j<=r} z_j``, ``N_r = (r + 1) - P_r``, ``I_r = G - P_r``, ``U_r = G + N_r`` (exact integer counts):
    ``g_r = J_r - J_{r-1}`` with ``J_r = 1 - I_r / U_r``, evaluated without the cancellation as ``1 / U_r`` where ``z_r = 1`` and
    ``I_r / ((U_r - 1) U_r)`` where ``z_r = 0``; with ``G = 0``: ``g_0 = 1`` and every other ``g_r = 0``.

    **Multiclass** (logits ``[B,K,H,W]``, target ``[B,H,W]`` or ``[B,1,H,W]``): ``p = softmax(x, dim=1)``; for class c and pixel i,
    ``z = [y_i == c]`` and ``e = |z - p_ic|``; ``L_c = sum_r e_(r) g_r``; the loss is the mean of ``L_c`` over the classes present
    among the valid pixels (``G_c > 0``), 0 if none is.  Gradient: ``dL_c/de_i = g_rank(i)`` (the coefficients are constants),
    ``de/dp = -1`` where z = 1 and ``+1`` where z = 0, exactly 0 where ``e == 0``, then back through the softmax.

    **Binary** (logits and target of equal numel and batch size, ``z = [y == 1]``, any other value that is not ``ignore_index``
    counts as 0): ``e = max(0, 1 - x (2z - 1))``, ``L = sum_r e_(r) g_r`` (also with ``G = 0``);
    ``dL/dx_i = -(2z - 1) g_rank(i)`` where ``e_i > 0`` and exactly 0 elsewhere.

    - A pixel with ``y == ignore_index`` (compared as int64) gets key 0 and label bit 0: it sorts behind every positive error, adds
      nothing to the loss and has an exactly zero gradient in every class -- the result of smp's compaction, without the pass.
    - A multiclass target outside ``0..K-1`` that is not ignored matches no class; the target is never used as an index.
    - ``per_image=False``: one segment of ``B H W`` per class.  ``per_image=True``: one segment of ``H W`` per image and class; the
      result is the mean over images of each image's mean over its present classes (binary: the mean over images).
    - NaN logits are unspecified.

    ``LowresLogits`` input is materialised (``reads_lowres`` is False for this loss); bf16 or non-contiguous logits are converted.
    ``mode="multilabel"`` and ``from_logits=False`` raise ``NotImplementedError``."""

    def __init__(self, mode: str, per_image: bool = False, ignore_index: int | None = None, from_logits: bool = True) -> None:
        super().__init__()
        _check_mode("LovaszLoss", mode)
        if not from_logits:
            raise NotImplementedError("gdlhip LovaszLoss implements from_logits=True only")
        ignore_index = _checked_ignore_index("LovaszLoss", ignore_index)
        self.mode, self.per_image, self.ignore_index, self.from_logits = mode, bool(per_image), ignore_index, True
        self.options = ops.LovaszOptions(self.per_image, ignore_index)

    def forward(self, y_pred, y_true: Tensor) -> Tensor:
        binary = self.mode == "binary"
        x, y_true, _ = _loss_input(y_pred, y_true, None, squeeze=not binary)      # (no low-resolution kernels: always the logits)
        if binary and (x.dim() < 1 or x.shape[0] != y_true.shape[0] or x.numel() != y_true.numel()):
            raise ValueError(f"LovaszLoss(binary): y_pred {tuple(x.shape)} and y_true {tuple(y_true.shape)} do not match")
        if not binary and x.dim() != 4:
            raise ValueError(f"LovaszLoss(multiclass): [B, K, H, W] logits expected (got {tuple(x.shape)})")
        return _Loss.apply("lovasz_binary" if binary else "lovasz", x, y_true.long().contiguous(), self.options, None, None)


def reads_lowres(loss, num_classes: int | None = None) -> bool:
    """True for a loss that evaluates itself (and its gradient) from ``LowresLogits``: a task may then ask the model for the heads'
    own maps instead of the resized [B, K, H, W] logits.  gdlhip's multiclass DiceLoss, JaccardLoss, TverskyLoss and FocalLoss,
    SoftCrossEntropyLoss and CrossEntropyLoss (gdlhip's, not torch's); for a one-class model (``num_classes == 1``) also their binary modes, which read the head's
    [B, h, w, 1] map, and SoftBCEWithLogitsLoss (which has no mode: its low-resolution kernels are the one-class ones)."""
    if isinstance(loss, (_DiceFamily, FocalLoss)):
        return loss.mode == "multiclass" or (loss.mode == "binary" and num_classes == 1)
    if isinstance(loss, SoftBCEWithLogitsLoss):
        return num_classes == 1
    return isinstance(loss, (SoftCrossEntropyLoss, CrossEntropyLoss))


def predict_mask(logits) -> Tensor:
    """``softmax(dim=1).argmax(dim=1)`` (segmentation_dofa.py:281).  For not-yet-resized logits (LowresLogits) the resize is
    evaluated per pixel inside the kernel: the same mask without the [B, K, H, W] tensor."""
    if isinstance(logits, LowresLogits):
        low = logits.low
        if low.dtype == torch.float32 and low.dim() == 4 and 2 <= low.shape[3] <= 16:
            return ops.upsample_argmax(low.contiguous(), logits.size)
        logits = logits.materialise()
    return ops.softmax_argmax(logits.float().contiguous())


def predict_binary_mask(logits, threshold: float = 0.5) -> Tensor:
    """``(out.sigmoid().squeeze(1) > threshold).long()`` (segmentation_dofa.py:279) for a one-class model: int64 [B, H, W].  For
    not-yet-resized logits (LowresLogits) the resize is evaluated per pixel inside the kernel; resized logits take one pass.
    A LowresLogits that is not f32, or whose shape ``ops.dice_lowres_ok`` rejects (a downsample, a factor above 64), is resized
    first (``materialise()``) and thresholded by ``sigmoid_threshold`` -- still HIP kernels, the same mask, as ``predict_mask``
    does for its shapes; it is the C entry point ``gdl_upsample_threshold`` and ``ops.upsample_threshold`` that refuse such a
    shape with an error.  More than one class is an error here too."""
    if isinstance(logits, LowresLogits):
        low = logits.low
        if low.dim() != 4 or low.shape[3] != 1:
            raise ValueError(f"predict_binary_mask: one-class logits [B, h, w, 1] expected, got {tuple(low.shape)}")
        size = (int(logits.size[0]), int(logits.size[1]))
        if low.dtype == torch.float32 and ops.dice_lowres_ok(low, size):
            return ops.upsample_threshold(low.contiguous(), size, threshold)
        logits = logits.materialise()
    if logits.dim() != 4 or logits.shape[1] != 1:
        raise ValueError(f"predict_binary_mask: one-class logits [B, 1, H, W] expected, got {tuple(logits.shape)}")
    return ops.sigmoid_threshold(logits.float().contiguous(), threshold)


@torch.no_grad()
def predict_probs(logits) -> Tensor:
    """``f.softmax(output, dim=1)`` (more than one class) / ``f.sigmoid(output)`` (one class) of the exported inference model
    (tools/script_model.py:54-58): f32 [B, K, H, W].  For not-yet-resized f32 logits (LowresLogits) with 1..16 classes the resize
    is evaluated per pixel inside the kernel: the same probabilities without the [B, K, H, W] logits.  Any other LowresLogits is
    resized first (``materialise()``), as ``predict_mask`` does for its shapes.  Inference only: no gradient."""
    if isinstance(logits, LowresLogits):
        low = logits.low
        if low.dtype == torch.float32 and low.dim() == 4 and 1 <= low.shape[3] <= 16:
            return ops.upsample_probs(low.contiguous(), (int(logits.size[0]), int(logits.size[1])))
        logits = LowresLogits(low.float().contiguous(), logits.size).materialise()      # (the resize kernel reads f32)
    return ops.class_probs(logits.float().contiguous())


# ------------------------------------------------------------------ optimizer
class _FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: one chunk table per param group (rows {param, grad, buf0, buf1, count, shadow}, cached on
    the addresses), the fused global-norm clip (Lightning's ``gradient_clip_val``), the bf16 GEMM operands rewritten by the
    update kernel, the one-launch rebuild of the derived operands, and the device-side state of the capturable form.  A subclass
    supplies the per-parameter state, the two buffer columns of a row, slots 2..5 of the device state and the two launches."""

    CHUNK = 65536

    def __init__(self, params, defaults: dict, max_grad_norm: float | None, capturable: bool) -> None:
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        # capturable (torch.optim.Adam(capturable=True)): step count, bias corrections and hyper-parameters live in device
        # memory, so that a hipGraph-captured step (gdlhip.graphs) replays correctly; chunk tables come from pinned memory
        self.capturable = capturable
        self._dev_state: dict = {}    # param group index -> f32[8] {step, lr, <four hyper-parameters>, <two slots the tick kernel derives>}
        self._dev_lr: dict = {}       # param group index -> the learning rate last written to the device state
        self._table_bufs: dict = {}   # param group index -> (pinned, device) chunk-table buffers, allocated once
        self._acc = None
        self._tables: dict = {}      # param group index -> (address signature, device chunk table)
        self.table_builds = 0        # how often a chunk table was (re)built: 1 per group in steady state
        # bf16 GEMM operands of the parameters (gemm_weight cache) are rewritten by the update kernel itself
        self.shadows = LAUNCH_FUSION
        self._shadowed: list = []
        self._repack = None          # (signature, device table, tiles) of the derived-operand rebuild (refresh_derived)
        self._derived_last: list = []   # (cache key, operand, parameter) of the last refresh_derived
        self._repack_scan = None     # ((operand builds so far, registered parameters, updated parameters), entries) of the last scan

    # ---- what a subclass supplies
    def _init_state(self, group: dict, p: Tensor, st: dict) -> None:
        """Create what is missing in the state of ``p`` (torch's key names; ``step`` is a host integer)."""
        raise NotImplementedError

    def _buffers(self, group: dict, st: dict) -> tuple:
        """Addresses for columns 2 and 3 of the parameter's chunk rows (0 = none)."""
        raise NotImplementedError

    def _dev_hyper(self, group: dict) -> list:
        """Slots 2..5 of the device state (slot 0 = step, 1 = lr; 6..7 are written by the tick kernel)."""
        raise NotImplementedError

    def _update(self, group: dict, table: Tensor, step: int, clip) -> None:
        """The update of one chunk table with host hyper-parameters."""
        raise NotImplementedError

    def _update_dev(self, group: dict, table: Tensor, state: Tensor, clip) -> None:
        """Tick + update of one chunk table with the hyper-parameters of the device state."""
        raise NotImplementedError

    def load_state_dict(self, state_dict) -> None:
        """torch's own optimizers keep ``step`` as a tensor: here it is a host integer (it keys the chunk tables)."""
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if isinstance(st.get("step"), Tensor):
                st["step"] = int(st["step"].item())

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        todo = [(gi, g, p) for gi, g in enumerate(self.param_groups) for p in g["params"] if p.grad is not None]
        if not todo:
            return loss
        dev = todo[0][2].device
        # one chunk table per (param group, step count) -> one launch each.  A table only holds addresses and sizes: it is
        # rebuilt (535 rows for DOFA-base + one H2D copy) only when a parameter, gradient or state buffer moved -- with
        # gradient_as_bucket_view / set_to_none=False and a caching allocator that is the first step only
        buckets: dict = {}
        shadowed: list = []
        for gi, group, p in todo:
            st = self.state[p]
            self._init_state(group, p, st)
            st["step"] += 1
            if p.grad.stride() != p.stride():
                p.grad = _restride(p.grad, p)
            _flat(p), _flat(p.grad)  # layout check (dense storage)
            sig = buckets.setdefault((gi, st["step"]), [])
            sh = gemm_weight_shadow(p) if self.shadows else None
            if sh is not None:
                shadowed.append((sh[0], sh[1], p))     # the tensor is held: the table's address stays valid
            sig.append((p.data_ptr(), p.grad.data_ptr(), *self._buffers(group, st), p.numel(),
                        0 if sh is None else sh[1].data_ptr()))
            mark_updated(p)
        tables = {}
        for key, sig in buckets.items():
            sig = tuple(sig)
            hit = self._tables.get(key[0])
            if hit is None or hit[0] != sig:
                rows = [(pp + 4 * off, gp + 4 * off, mp + 4 * off if mp else 0, vp + 4 * off if vp else 0, min(self.CHUNK, n - off),
                         sp + 2 * off if sp else 0)
                        for pp, gp, mp, vp, n, sp in sig for off in range(0, n, self.CHUNK)]
                host = torch.tensor(rows, dtype=torch.int64)
                hit = (sig, self._upload(key[0], host, dev))
                if len(buckets) == len({k[0] for k in buckets}):      # (one step count per group: the usual case -> cacheable)
                    self._tables[key[0]] = hit
                self.table_builds += 1
            tables[key] = hit[1]
        clip = None
        if self.max_grad_norm is not None:
            if self._acc is None:
                self._acc = torch.zeros(2, device=dev, dtype=torch.float32)
            self._acc.zero_()
            for t in tables.values():
                ops.multi_sumsq(t, self._acc[0:1])
            ops.clip_coef(self._acc[0:1], float(self.max_grad_norm), self._acc[1:2])
            clip = self._acc[1:2]
        if self.capturable and not torch.cuda.is_current_stream_capturing():
            self.sync_lr()                # a scheduler's param_groups["lr"] write reaches the device-side hyper-parameters
        for (gi, step), t in tables.items():
            group = self.param_groups[gi]
            if self.capturable:
                self._update_dev(group, t, self.device_state(gi, dev), clip)
            else:
                self._update(group, t, step, clip)
        self._shadowed = shadowed
        for key, val, p in shadowed:      # the kernels above rewrote the bf16 GEMM operands too
            refresh_shadow(key, val, p)
        if self.shadows:
            self.refresh_derived([p for _, _, p in todo], dev)
        return loss

    def _upload(self, name, host: Tensor, dev) -> Tensor:
        """A host int64 table on the device.  capturable: under stream capture nothing may be allocated (pinned or device), so
        both buffers exist since the first table of this name and shape; the captured H2D copy re-reads the pinned one at
        every replay."""
        if not self.capturable:
            return host.to(dev, non_blocking=True)
        bufs = self._table_bufs.get(name)
        if bufs is None or bufs["dev"].shape != host.shape:
            pin = lambda: torch.empty(host.shape, dtype=torch.int64).pin_memory()      # noqa: E731
            bufs = {"eager": [pin(), pin()], "events": [None, None], "capture": pin(), "i": 0,
                    "dev": torch.empty(host.shape, dtype=torch.int64, device=dev)}
            self._table_bufs[name] = bufs
        if torch.cuda.is_current_stream_capturing():
            # the captured H2D copy re-reads this pinned buffer at every replay: eager rebuilds never touch it
            src = bufs["capture"]
            src.copy_(host)
            bufs["dev"].copy_(src, non_blocking=True)
        else:
            # eager steps with set_to_none gradients rebuild the table every step; its asynchronous H2D copy reads
            # the pinned buffer later, so the host alternates between two and only waits for the copy issued two
            # rebuilds ago (long done) instead of overwriting a buffer whose copy has not run yet
            i = bufs["i"] = bufs["i"] ^ 1
            if bufs["events"][i] is not None:
                bufs["events"][i].synchronize()
            src = bufs["eager"][i]
            src.copy_(host)
            bufs["dev"].copy_(src, non_blocking=True)
            ev = bufs["events"][i] or torch.cuda.Event()
            ev.record()
            bufs["events"][i] = ev
        return bufs["dev"]

    @torch.no_grad()
    def refresh_derived(self, params=None, dev=None) -> int:
        """Rebuild, in ONE launch (gdl_multi_repack), every bf16 operand that was derived from the given (default: all) conv
        parameters in another element order and sits in the operand cache -- channel slices and tap-major forms of the 3x3
        parameters, data-gradient operands -- and mark the entries current.  Called behind every update; GraphedTrainStep calls
        it after restoring the parameters.  Returns the number of operands rewritten."""
        everything = params is None
        if everything:
            params = [p for g in self.param_groups for p in g["params"]]
        # steady state: nothing was built since the last scan (the entries were rewritten in place and revalidated), the same
        # parameters were updated -> the same entries, no scan
        scan_key = (_CACHE_BUILDS[0], len(_DERIVED), len(params))
        if not everything and self._repack_scan is not None and self._repack_scan[0] == scan_key:
            ents = self._repack_scan[1]
        else:
            ents = [(p, *e) for p in params for e in derived_operands(p)]
            self._repack_scan = None if everything else (scan_key, ents)
        if not ents:
            return 0
        dev = dev or ents[0][0].device
        sig = tuple((p.data_ptr(), val.data_ptr(), mode, c0, c1) for p, _, val, mode, c0, c1 in ents)
        hit = self._repack
        # (inside a stream capture the table is ALWAYS uploaded: the captured copy then restores it from its own pinned buffer
        # at every replay, whatever eager steps in between wrote into the device buffer -- like the update's chunk tables, whose
        # gradient addresses change with every capture)
        if hit is None or hit[0] != sig or (self.capturable and torch.cuda.is_current_stream_capturing()):
            rows, tile0 = [], 0
            for p, _, val, mode, c0, c1 in ents:
                n, c, t = p.shape[0], p.shape[1], p.shape[2] * p.shape[3]
                cs = c1 - c0
                if val.numel() != n * t * cs:
                    msg = f"gdlhip {type(self).__name__}: derived operand {tuple(val.shape)} does not match parameter {tuple(p.shape)}[{c0}:{c1}]"
                    raise ValueError(msg)
                tiles_c = (cs + 31) // 32
                rows.append((p.data_ptr(), val.data_ptr(), n, t, c, c0, cs, mode, tile0, tiles_c))
                tile0 += t * ((n + 31) // 32) * tiles_c
            hit = self._repack = (sig, self._upload("repack", torch.tensor(rows, dtype=torch.int64), dev), tile0)
        ops.multi_repack(hit[1], hit[2])
        for p, key, val, _, _, _ in ents:
            refresh_shadow(key, val, p)
        self._derived_last = [(key, val, p) for p, key, val, _, _, _ in ents]
        return len(ents)

    def device_state(self, gi: int, dev=None) -> Tensor:
        """The device-side f32[8] state of param group gi (capturable mode; Adam / AdamW: {step, lr, b1, b2, eps, wd, bc1, bc2}),
        created from the group's current hyper-parameters on first use.  A scheduler's new learning rate reaches a captured step
        through sync_lr()."""
        st = self._dev_state.get(gi)
        if st is None:
            g = self.param_groups[gi]
            steps = {self.state[p]["step"] - 1 for p in g["params"] if p in self.state and self.state[p]}
            step0 = float(steps.pop()) if len(steps) == 1 else 0.0
            st = torch.tensor([step0, g["lr"], *self._dev_hyper(g), 0.0, 0.0], dtype=torch.float32).to(dev)
            self._dev_state[gi] = st
            self._dev_lr[gi] = float(g["lr"])
        return st

    def sync_lr(self) -> None:
        """Write the param groups' current learning rates into the device state when a scheduler changed them (one fill_ on the
        stream per changed group, nothing otherwise).  Capturable mode reads lr from the device: called at the start of every
        eager step and by GraphedTrainStep before every replay."""
        for gi, st in self._dev_state.items():
            lr = float(self.param_groups[gi]["lr"])
            if self._dev_lr.get(gi) != lr:
                st[1:2].fill_(lr)
                self._dev_lr[gi] = lr

    def note_replay(self) -> None:
        """A captured step ran: advance the host-side step counts (what state_dict() / checkpoints report) like the device's."""
        for g in self.param_groups:
            for p in g["params"]:
                st = self.state.get(p)
                if st:
                    st["step"] += 1


class _FusedAdamBase(_FusedOptimizer):
    """Adam and AdamW: the same state, rows and device state; they differ in the kernel instantiation only."""

    def __init__(self, params, lr, betas, eps, weight_decay, max_grad_norm, capturable) -> None:
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), max_grad_norm, capturable)

    def _init_state(self, group, p, st) -> None:
        if not st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _buffers(self, group, st) -> tuple:
        return st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()

    def _dev_hyper(self, group) -> list:
        return [*group["betas"], group["eps"], group["weight_decay"]]


class FusedAdam(_FusedAdamBase):
    """torch.optim.Adam semantics with the update (and optional global-norm clipping, Lightning's
    ``gradient_clip_val``) done by HIP kernels.  Reference: configs/dofa_config_RGB.yaml:11,62-65."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm: float | None = None, capturable: bool = False) -> None:
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, capturable)

    def _update(self, group, table, step, clip) -> None:
        ops.multi_adam(table, group["lr"], *group["betas"], group["eps"], group["weight_decay"], step, clip)

    def _update_dev(self, group, table, state, clip) -> None:
        ops.adam_tick(state, *group["betas"])
        ops.multi_adam_dev(table, state, clip)


class FusedAdamW(_FusedAdamBase):
    """torch.optim.AdamW semantics (decoupled weight decay: the parameter is scaled by ``1 - lr * weight_decay``, the moments
    see the gradient alone) on the FusedAdam machinery: one launch per param group, fused clip, bf16 operands rewritten by the
    update, capturable.  With ``weight_decay=0`` the results are FusedAdam's bits."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: float | None = None, capturable: bool = False) -> None:
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, capturable)

    def _update(self, group, table, step, clip) -> None:
        ops.multi_adamw(table, group["lr"], *group["betas"], group["eps"], group["weight_decay"], step, clip)

    def _update_dev(self, group, table, state, clip) -> None:
        ops.adam_tick(state, *group["betas"])
        ops.multi_adamw_dev(table, state, clip)


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD semantics (momentum, dampening, nesterov, weight decay) on the FusedAdam machinery.  State keys are
    torch's: ``momentum_buffer`` (absent when the group's momentum is 0) plus an integer ``step``.  The momentum buffer of a
    parameter's first step is the gradient itself, dampening not applied; the kernel takes that from the step count (capturable:
    from the group's device-side count, as the Adam bias corrections do), never from a zero-filled buffer."""

    def __init__(self, params, lr: float, momentum: float = 0, dampening: float = 0, weight_decay: float = 0,
                 nesterov: bool = False, max_grad_norm: float | None = None, capturable: bool = False) -> None:
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov),
                         max_grad_norm, capturable)

    def _init_state(self, group, p, st) -> None:
        if group["momentum"] != 0 and st.get("momentum_buffer") is None:
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] = 0
        # (a state written by torch.optim.SGD has a buffer and no count: whatever its count, the first step is behind it)
        st.setdefault("step", 1 if "momentum_buffer" in st else 0)

    def _buffers(self, group, st) -> tuple:
        buf = st.get("momentum_buffer") if group["momentum"] != 0 else None
        return (0 if buf is None else buf.data_ptr()), 0

    def _dev_hyper(self, group) -> list:
        return [group["momentum"], group["dampening"], float(bool(group["nesterov"])), group["weight_decay"]]

    def _update(self, group, table, step, clip) -> None:
        ops.multi_sgd(table, group["lr"], group["momentum"], group["dampening"], group["nesterov"], group["weight_decay"], step, clip)

    def _update_dev(self, group, table, state, clip) -> None:
        ops.sgd_tick(state)
        ops.multi_sgd_dev(table, state, clip)


def _flat(t: Tensor) -> Tensor:
    """The dense storage of a (possibly channels_last) tensor, as a flat view."""
    if t.is_contiguous():
        return t.view(-1)
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return t.permute(0, 2, 3, 1).reshape(-1)
    msg = f"gdlhip fused optimizer: parameter layout {t.stride()} is not dense"
    raise ValueError(msg)


def _restride(g: Tensor, p: Tensor) -> Tensor:
    out = torch.empty_like(p, memory_format=torch.preserve_format)
    out.copy_(g)
    return out
