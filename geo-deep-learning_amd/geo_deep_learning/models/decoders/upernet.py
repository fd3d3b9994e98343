"""UperNet decoder on MI355X (drop-in for the reference's models/decoders/upernet.py)."""

from __future__ import annotations

import torch
from torch import nn

from geo_deep_learning.models.utils import PPM, ConvModule
from gdlhip import nn as gnn
from gdlhip import ops


class UperNetDecoder(nn.Module):
    """PPM + FPN decoder (upernet.py:9-152), with or without the scale_modules pyramid (upernet.py:37-54)."""

    def __init__(self, embed_dim: list[int], pool_scales: tuple[int, ...] = (1, 2, 3, 6), channels: int = 256,
                 *, align_corners: bool = True, scale_modules: bool = False) -> None:
        super().__init__()
        if align_corners:
            msg = "gdlhip UperNetDecoder: align_corners=True is not on the hot path (dofa.py:66)"
            raise NotImplementedError(msg)
        self.scale_modules = scale_modules
        if scale_modules:
            # upernet.py:37-54: the pyramid is built inside the decoder from four equal-resolution taps (plain ViT encoders).
            # Plain torch containers: state-dict keys / shapes of the reference, and convert_sync_batchnorm finds fpn1.1
            self.fpn1 = nn.Sequential(nn.ConvTranspose2d(embed_dim[0], embed_dim[0] // 2, 2, 2), nn.BatchNorm2d(embed_dim[0] // 2),
                                      nn.GELU(), nn.ConvTranspose2d(embed_dim[0] // 2, embed_dim[0] // 4, 2, 2))
            self.fpn2 = nn.Sequential(nn.ConvTranspose2d(embed_dim[1], embed_dim[1] // 2, 2, 2))
            self.fpn3 = nn.Sequential(nn.Identity())
            self.fpn4 = nn.Sequential(nn.MaxPool2d(kernel_size=2, stride=2))
            self.embed_dim = [embed_dim[0] // 4, embed_dim[1] // 2, embed_dim[2], embed_dim[3]]
        else:
            self.embed_dim = embed_dim
        self.out_channels = channels
        self.channels = channels
        self.align_corners = align_corners
        self.psp_modules = PPM(pool_scales, self.embed_dim[-1], self.channels, align_corners=align_corners)
        self.bottleneck = ConvModule(self.embed_dim[-1] + len(pool_scales) * self.channels, self.channels, 3,
                                     padding=1, inplace=True)
        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        for embed_dim_ in self.embed_dim[:-1]:
            self.lateral_convs.append(ConvModule(embed_dim_, self.channels, 1, inplace=False))
            self.fpn_convs.append(ConvModule(self.channels, self.channels, 3, padding=1, inplace=False))
        self.fpn_bottleneck = ConvModule(len(self.embed_dim) * self.channels, self.channels, 3, padding=1,
                                         inplace=True)

    def psp_forward_nhwc(self, x: torch.Tensor) -> torch.Tensor:
        """upernet.py:103-109: cat([x, up(ppm_s(x))...]) -> 3x3 bottleneck; the upsample writes
        straight into the concat buffer."""
        size = (x.shape[1], x.shape[2])
        cat = gnn.concat_upsample([x, *self.psp_modules.forward_nhwc_lowres(x)], size)
        return self.bottleneck.forward_nhwc(cat)

    def scale_inputs_nhwc(self, inputs: list[torch.Tensor]) -> list[torch.Tensor]:
        """upernet.py:113-119: x4 (ConvTranspose -> BN -> GELU -> ConvTranspose), x2 (ConvTranspose), x1, x1/2 (2x2 max-pool)."""
        half = gnn.conv_transpose2x2_bn_gelu(inputs[0], self.fpn1[0], self.fpn1[1])
        return [gnn.conv_transpose2x2(half, self.fpn1[3]), gnn.conv_transpose2x2(inputs[1], self.fpn2[0]), inputs[2],
                gnn.maxpool2x2(inputs[3])]

    def tail_fusable(self, inputs: list[torch.Tensor], head_conv: nn.Conv2d) -> bool:
        """True when ``forward_nhwc(inputs, head_conv=head_conv)`` can hand the 1x1 head's logits back without writing the
        normalised ``fpn_bottleneck`` output (gdlhip.nn.bn_tail_fusable: bf16 training step, statistics of one process)."""
        if self.scale_modules:      # (the output size is that of the scaled inputs[0]; DOFA's decoder has no scale_modules: not wired)
            return False
        x = inputs[0]
        return gnn.bn_tail_fusable((x.shape[0], x.shape[1], x.shape[2], self.channels), x.dtype, self.fpn_bottleneck.norm, head_conv)

    def forward_nhwc(self, inputs: list[torch.Tensor], head_conv: nn.Conv2d | None = None) -> torch.Tensor:
        """``head_conv`` (only where ``tail_fusable``): the [B, H, W, K] f32 logits of that 1x1 head over the decoder output are
        returned instead of the output itself."""
        if self.scale_modules:
            inputs = self.scale_inputs_nhwc(inputs)
        # lateral 1x1 convolutions and the PPM branches are independent: one group (one SyncBatchNorm message per direction)
        # a lateral's only consumer is its top-down add: with statistics of one process (no group message to share) each lateral
        # runs inside the add's node, which applies BatchNorm + ReLU on load (gnn.conv_bn_act_upsample_add, GDL_FUSE_BN_TAIL)
        lat_in_add = gnn.FUSE_BN_TAIL and all(gnn.single_process_bn_train(m.norm) for m in self.lateral_convs)
        lat_items = [] if lat_in_add else [dict(x=inputs[i], conv=m.conv, norm=m.norm) for i, m in enumerate(self.lateral_convs)]
        ppm_items = self.psp_modules.items_nhwc(inputs[-1])
        res = gnn.conv_bn_act_group(lat_items + ppm_items)
        laterals = res[:len(lat_items)] if not lat_in_add else [None] * len(self.lateral_convs)
        x = inputs[-1]
        cat = gnn.concat_upsample([x, *res[len(lat_items):]], (x.shape[1], x.shape[2]))      # upernet.py:103-109
        laterals.append(self.bottleneck.forward_nhwc(cat))
        n = len(laterals)
        for i in range(n - 1, 0, -1):  # top-down: lat[i-1] += up(lat[i])
            if lat_in_add:
                m = self.lateral_convs[i - 1]
                laterals[i - 1] = gnn.conv_bn_act_upsample_add(inputs[i - 1], m.conv, m.norm, laterals[i])
            else:
                laterals[i - 1] = gnn.upsample_add(laterals[i - 1], laterals[i])
        fpn_outs = gnn.conv_bn_act_group([dict(x=laterals[i], conv=self.fpn_convs[i].conv, norm=self.fpn_convs[i].norm)
                                          for i in range(n - 1)])
        fpn_outs.append(laterals[-1])
        size = (fpn_outs[0].shape[1], fpn_outs[0].shape[2])
        # 3x3 bottleneck over the concat of the upsampled levels; in training the upsampled levels' gradients are computed at
        # their own resolution (gdlhip.nn.concat_resize_conv_bn_act)
        return gnn.concat_resize_conv_bn_act(fpn_outs, self.fpn_bottleneck.conv, self.fpn_bottleneck.norm,
                                             relu=self.fpn_bottleneck.act is not None, head_conv=head_conv)

    def forward(self, inputs: list[torch.Tensor]) -> torch.Tensor:
        cd = gnn.compute_dtype()
        xs = [gnn.to_compute(ops.as_nhwc(x), cd) for x in inputs]
        return ops.as_nchw(self.forward_nhwc(xs))
