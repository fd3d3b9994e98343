"""Inference wrappers (drop-in for the reference's tools/script_model.py:10-86): raw tile in, class probabilities out.
The reference traces the model with ``torch.jit``; the HIP model is a sequence of C-ABI kernel launches and needs no
tracing, so the wrapper only fixes the pre/post-processing: ``normalization`` (the caller's ``image_min`` / ``image_max`` ->
``norm_min`` / ``norm_max``) and ``(x-mean)/std`` in one fused normalise kernel, the model under ``no_grad`` (bf16 autocast
optional), softmax / sigmoid in one kernel -- straight from the head's low-resolution map where the model can hand it over
(``forward(..., lowres_logits=True)``: the resized [B, K, H, W] logits are then never written)."""

from __future__ import annotations

import inspect

import torch
from torch import nn

from gdlhip import nn as gnn
from gdlhip import ops

_DEFAULT_RANGE = (0, 255, 0.0, 1.0)


def _takes_lowres_logits(model: nn.Module) -> bool:
    try:
        return "lowres_logits" in inspect.signature(model.forward).parameters
    except (TypeError, ValueError):
        return False


class ScriptModel(nn.Module):
    """tools/script_model.py:10-60."""

    def __init__(self, model: nn.Module, device: torch.device | None = None, num_classes: int = 1,
                 input_shape: tuple[int, int, int, int] = (1, 3, 512, 512), mean: list[float] | None = None,
                 std: list[float] | None = None, image_min: int = 0, image_max: int = 255, norm_min: float = 0.0,
                 norm_max: float = 1.0, *, from_logits: bool = True, bf16: bool = False) -> None:
        super().__init__()
        self.image_min, self.image_max = int(image_min), int(image_max)
        self.norm_min, self.norm_max = float(norm_min), float(norm_max)
        if self.image_max == self.image_min:
            msg = f"ScriptModel: image_max == image_min ({self.image_min}): the input range is empty"
            raise ValueError(msg)
        self.device = device or torch.device("cuda")
        self.num_classes, self.from_logits, self.bf16 = num_classes, from_logits, bf16
        c = input_shape[1]
        self.register_buffer("mean", torch.tensor(mean or [0.0] * c, dtype=torch.float32))
        self.register_buffer("std", torch.tensor(std or [1.0] * c, dtype=torch.float32))
        self.model = model.eval()
        # a model that can return its heads' own maps (gdlhip.nn.LowresLogits): the probabilities are computed from them
        self.lowres = _takes_lowres_logits(self.model)
        self.to(self.device)

    def _normalize(self, x: torch.Tensor) -> torch.Tensor:
        rng = (self.image_min, self.image_max, self.norm_min, self.norm_max)
        if rng == _DEFAULT_RANGE:       # the reference defaults: the /255 kernel the datamodule uses
            return ops.normalize_raw(x, self.mean, self.std)
        return ops.normalize_range(x, self.mean, self.std, *rng)

    def _call(self, *args: torch.Tensor):
        return self.model(*args, lowres_logits=True) if self.lowres else self.model(*args)

    def _logits(self, x: torch.Tensor):
        return self._call(x)

    def raw_output(self, x: torch.Tensor):
        """The model's own output for tiles that are normalised already (``gdlhip.nn.LowresLogits`` where the model hands its
        heads' maps over, otherwise the resized logits): what ``forward`` turns into probabilities, and what whole-scene
        inference (tools/scene_inference.py) stitches without them."""
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.bf16):
            return self._logits(x)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x.to(self.device)
        if x.dtype not in (torch.uint8, torch.uint16, torch.int16):
            x = x.float()
        out = self.raw_output(self._normalize(x.contiguous()))
        with torch.no_grad():
            if self.from_logits:
                return gnn.predict_probs(out)
            # the reference returns the resized logits here
            return out.materialise() if isinstance(out, gnn.LowresLogits) else out


class SegmentationScriptModel(ScriptModel):
    """tools/script_model.py:63-86: the model returns (out, aux) and the wrapper takes the main output only; ``wavelengths``
    are fixed at export time for DOFA."""

    def __init__(self, model: nn.Module, wavelengths: torch.Tensor | None = None, **kwargs: object) -> None:
        super().__init__(model, **kwargs)
        self.wavelengths = wavelengths

    def _logits(self, x: torch.Tensor):
        out = self._call(x) if self.wavelengths is None else self._call(x, self.wavelengths)
        # (out, aux): the aux head's map is dropped unresized.  A bare LowresLogits is a tuple too: it is the output itself
        return out[0] if isinstance(out, tuple) and not isinstance(out, gnn.LowresLogits) else out
