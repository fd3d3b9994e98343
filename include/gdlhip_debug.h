/* gdlhip_debug.h -- the A/B and tuning hooks of libgdlhip.so.  NOT part of the public C ABI (include/gdlhip.h): tests, the
 * tools/ scripts and the GDL_* environment variables read by gdlhip/_lib.py are their only callers, and any of them may go
 * when the experiment it served is settled.  Each hook sets a process-wide switch that the host-side kernel selection reads;
 * none launches anything.  csrc/gdl_common.h includes this file, so the compiler checks every definition against it, and
 * gdlhip/_lib.py binds the hooks from it (DEBUG_SIGNATURES) with the parser that reads the public header: the same narrow
 * C dialect applies.
 */
#ifndef GDLHIP_DEBUG_H_
#define GDLHIP_DEBUG_H_

#ifdef __cplusplus
extern "C" {
#endif

/* ---- implicit-GEMM convolution (conv_gemm.hip): which tile variant gdl_conv_gemm_plan may pick ---- */
/* -1 = the planner's choice (default), otherwise the variant number of gdl_conv_gemm_plan for every call */
void gdl_debug_force_conv_variant(int v);
/* 0 = never pick the 3x3 shared-staging kernel (variant 4) */
void gdl_debug_set_conv_sf(int on);
/* 0 = never pick the direct narrow 3x3 kernel (variant 7) */
void gdl_debug_set_conv_narrow(int on);
/* 0 = never pick the dual-resident 256 x 128 tile (variant 6) */
void gdl_debug_set_conv_dual(int on);
/* 0 = never pick the four-stage 64^2 tile (variant 12: few tiles, long K) */
void gdl_debug_set_conv_stage4(int on);
/* 0 = never pick the one-wave-per-SIMD 256^2 tile (variant 8) */
void gdl_debug_set_conv_w4(int on);
/* 0 = never pick the persistent 256^2 tile for dense 1x1 layers (variant 9) */
void gdl_debug_set_conv_persist(int on);
/* the persistent 256^2 tile with deferred stores (variant 10, conv_gemm_w4p.hip): 0 = never (default), 1 = where it applies,
 * a value above 1 = on, and that value is the smallest N that takes it */
void gdl_debug_set_conv_w4p(int on);
/* weight KiB one N-tile group of the GEMM tile order may hold; 0 = no grouping */
void gdl_debug_set_conv_ngroup_kb(int kb);
/* 0 = the first epilogue of the 256^2 tiles instead of the coalesced one */
void gdl_debug_set_conv_epilogue(int v2);
/* 0 = no tap packing of the narrow-output 256x64 tile (variant 5) */
void gdl_debug_set_conv_tap_packing(int on);
/* 0 = channel-inner instead of tap-inner K order */
void gdl_debug_set_conv_korder(int tap_inner);
/* experiment bits handed to the GEMM kernels as `dbg` (0 = none) */
void gdl_debug_set_conv_dbg(int mode);
/* device buffer the GEMM kernels write per-workgroup cycle and real-time counters to (tools/probe_*.py size it); NULL = off */
void gdl_debug_set_conv_probe(void* dev_buf_2048x2_u64);

/* ---- weight gradient (wgrad.hip) ---- */
/* kernel-selection bits: 1 = never the 256^2 kernel (128^2 tiles only), 2 = never the row-segment kernel, 8 = N, C >= 256
 * layers on the 256^2 per-tap kernel */
void gdl_debug_force_wgrad_small(int on);
/* 1 = the register-transpose kernel for every call */
void gdl_debug_force_wgrad_v1(int on);
/* 1 = the first split-K rule of the 256^2 kernel */
void gdl_debug_set_wgrad_old_splits(int on);
/* XCDs (1, 2, 4; anything else = all 8) the tiles of a pixel range of the 256^2 kernel are dealt to */
void gdl_debug_set_wgrad_xcd_group(int g);
/* 1 = all tiles of a pixel range of the row-segment kernel on one XCD */
void gdl_debug_set_wgrad_rows_xcd(int on);

/* ---- attention (attention_v2.hip) ---- */
/* forward version (2 = 64-query waves; negative = the default) and the slack of its deferred running maximum
 * (default 6; 0 = the exact online softmax) */
void gdl_debug_set_flash_fwd(int version, float defer);

/* ---- resampling (resample.hip) and the low-resolution 3x3 forms (gather_mfma: resize_conv_bwd.hip; tapsum_*: resize_conv_fwd.hip) ---- */
/* 1 = the flat-index resize / pooling kernels for every shape */
void gdl_debug_set_flat_resample(int on);
/* 0 = the VALU gathers of the low-resolution backward instead of the one-pass matrix-core form */
void gdl_debug_set_gather_mfma(int on);
/* forward gather-sum: 0 = the pixel-by-pixel kernel, 1 = MFMA with the version chosen by shape (default), 5 = version 2
 * (4 x 16 pixel blocks, all channels, pipelined), 2 / 4 = version 1 (32- / 16-column blocks x 64 channels) */
void gdl_debug_set_tapsum_mfma(int mode);
/* forward gather-sum, pixel-by-pixel kernel: 4 = 8-byte bf16 vectors per thread, 8 = 16-byte ones, 0 = by shape */
void gdl_debug_set_tapsum_vec(int vec);
/* 0 = one workgroup per patch in the forward gather-sum instead of persistent workgroups */
void gdl_debug_set_tapsum_persist(int on);
/* 0 = versions 1 / 2 of the forward gather-sum where the rolling-row-window one applies */
void gdl_debug_set_tapsum_roll(int on);

/* ---- BatchNorm, classifier head, losses ---- */
/* 0 = the 8-byte / 256-channel mapping of the BatchNorm backward for every shape (norm.hip) */
void gdl_debug_set_bn_wide(int on);
/* 0 = the wave-per-pixel classifier-head kernels instead of the MFMA ones (head.hip) */
void gdl_debug_set_head_mfma(int on);
/* 0 = the gather kernel for every class count in the low-resolution Dice-family backward (loss_dice.hip) */
void gdl_debug_set_dice_lowres_tiled(int on);
/* 0 = the gather kernel for every class count in the low-resolution soft cross-entropy backward (loss_ce.hip) */
void gdl_debug_set_soft_ce_lowres_tiled(int on);

#ifdef __cplusplus
}
#endif
#endif /* GDLHIP_DEBUG_H_ */
