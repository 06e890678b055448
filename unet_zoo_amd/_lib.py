"""ctypes binding of libunetzoo_hip.so (C ABI declared in include/unetzoo_hip.h).

The product path has no CPU or PyTorch fallback: if the shared library is missing, or an op is
handed a non-CUDA tensor, it raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"``
(or ``make -C unet_zoo_amd/csrc``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_void_p

import torch

UZ_F32, UZ_BF16 = 0, 1
TAPS_CONV, TAPS_GATHER2X2, TAPS_CONV_UP2, TAPS_CONV_S2 = 0, 1, 2, 3
STORE_PLAIN, STORE_SHUFFLE2X2 = 0, 1
PACK_CONV_FWD, PACK_CONV_DGRAD, PACK_CONVT_FWD, PACK_CONVT_DGRAD, PACK_IM2COL, PACK_VEC_REPEAT = range(6)

LIB_NAME = "libunetzoo_hip.so"
# UNET_ZOO_AMD_LIB: another build of the same ABI (tools/kbench.py points it at the ablation build); the product
# never sets it, and bench.py refuses a library whose uz_build_ablate() is 1
LIB_PATH = os.environ.get("UNET_ZOO_AMD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

# every symbol include/unetzoo_hip.h declares (tests check the .so exports all of them)
EXPORTS = (
    "uz_abi_version", "uz_last_error_string", "uz_build_ablate", "uz_source_hash", "uz_set_cu_reserve", "uz_get_cu_reserve", "uz_clock_probe", "uz_conv_igemm_grid_m", "uz_conv_igemm",
    "uz_wgrad_split", "uz_wgrad_workspace_bytes", "uz_wgrad", "uz_wgrad_kernel_name", "uz_wgrad_phase", "uz_wgrad_xf_supported", "uz_wgrad_xf", "uz_conv3x3_first_supported", "uz_conv3x3_first_rows", "uz_conv3x3_first_fwd",
    "uz_conv3x3_first_wgrad_workspace_bytes", "uz_conv3x3_first_wgrad", "uz_conv3x3_first_wgrad_bn", "uz_pack_weights", "uz_pack_weights_batched", "uz_pack_conv3x3_batched", "uz_im2col3x3_nchw", "uz_bn_finalize",
    "uz_bn_eval_scale", "uz_bn_relu_apply", "uz_bn_relu_bwd_workspace_bytes", "uz_bn_relu_bwd_reduce", "uz_bn_relu_bwd_apply",
    "uz_outconv_fwd", "uz_outconv_fwd_xf", "uz_outconv_bwd_workspace_bytes", "uz_outconv_bwd", "uz_outconv_bwd_rows", "uz_outconv_bwd_bnred", "uz_bn_relu_bwd_apply_head_supported", "uz_bn_relu_bwd_apply_head",
    "uz_head_wide_supported", "uz_head_wide_grid", "uz_head_wide_fwd", "uz_head_wide_bwd_workspace_bytes", "uz_head_wide_bwd",
    "uz_colsum",
    "uz_attn_grid", "uz_attn_psi_fwd", "uz_attn_gate_fwd", "uz_attn_bwd_psi", "uz_attn_bwd_reduce",
    "uz_attn_bwd_apply", "uz_sum_rows", "uz_sum_rows_f32", "uz_sum2x2",
    "uz_bn_relu_add_apply", "uz_bn_relu_add_apply_fin", "uz_bn_relu_bwd_reduce_rows", "uz_bn_relu_bwd_apply_fin", "uz_bilinear_fwd", "uz_bilinear_bwd", "uz_resize_bilinear_fwd", "uz_resize_bilinear_bwd", "uz_resample2",
    "uz_pool_grad_combine",
    "uz_sideconv3x3_fwd", "uz_sideconv3x3_bwd_workspace_bytes", "uz_sideconv3x3_bwd",
    "uz_fuse1x1_fwd", "uz_fuse1x1_bwd_workspace_bytes", "uz_fuse1x1_bwd",
    "uz_conv_igemm_workspace_bytes", "uz_conv_igemm_ws_grid_m", "uz_conv_igemm_ws",
    "uz_conv_igemm_bnred_supported", "uz_conv_igemm_bnred", "uz_conv_igemm_xf_supported", "uz_conv_igemm_xf", "uz_conv_igemm_kernel_name", "uz_bn_bwd_finalize", "uz_profile_arm", "uz_profile_disarm",
    "uz_patchify", "uz_layernorm_fwd", "uz_layernorm_bwd_rows", "uz_layernorm_bwd", "uz_layernorm_act_bwd",
    "uz_ln_head_fwd", "uz_ln_head_bwd_workspace_bytes", "uz_ln_head_bwd", "uz_sum_rows_f32_ld",
    "uz_winattn_fwd", "uz_winattn_bwd_rows", "uz_winattn_bwd",
    "uz_colsum_workspace_bytes", "uz_colsum_ws", "uz_colstats_rows", "uz_colstats", "uz_cpb_fwd", "uz_cpb_bwd",
    "uz_cpb_fwd_batched", "uz_cpb_bwd_batched_workspace_bytes", "uz_cpb_bwd_batched",
    "uz_clip_adamw_workspace_bytes", "uz_clip_adamw",
    "uz_tail_workspace_bytes", "uz_tail_step", "uz_tail_accumulate", "uz_tail_swap",
    "uz_gelu_fwd", "uz_gelu_bwd", "uz_dwconv3x3", "uz_dwconv3x3_wgrad_rows", "uz_dwconv3x3_wgrad",
    "uz_space_to_depth", "uz_space_to_depth_crop", "uz_im2col_nchw", "uz_sra_fwd", "uz_sra_bwd_workspace_bytes", "uz_sra_bwd",
    "uz_bce_dice_workspace_bytes", "uz_bce_dice", "uz_colsum_batched_workspace_bytes", "uz_colsum_batched", "uz_sum_rows_f32_batched", "uz_conv_igemm_res", "uz_wgrad_multi_workspace_bytes", "uz_wgrad_multi", "uz_conv_igemm_res_ws",
    "uz_add_relu", "uz_relu_bwd", "uz_pil_resample_h_u8", "uz_pil_resample_v_f32",
    "uz_gemm_nt", "uz_softmax_fwd", "uz_softmax_bwd", "uz_adaptive_avgpool_fwd", "uz_adaptive_avgpool_bwd",
    "uz_rowdot_f32", "uz_cast_rows", "uz_wgrad_batched_workspace_bytes", "uz_wgrad_batched", "uz_wgrad_batched2",
    "uz_softmax_workspace_bytes", "uz_add_map", "uz_dropout", "uz_chanscale_relu", "uz_chanattn_probs_fwd", "uz_chanattn_probs_bwd",
    "uz_conv5x5_grid_m", "uz_conv5x5", "uz_wgrad5x5_workspace_bytes", "uz_wgrad5x5",
    "uz_bn_elu_apply", "uz_bn_elu_bwd_rows", "uz_bn_elu_bwd_reduce", "uz_bn_elu_bwd_apply",
    "uz_conv_igemm_bnact_supported", "uz_conv_igemm_bnact", "uz_conv3x3_first_fwd_bnact",
    "uz_region_loss_workspace_bytes", "uz_region_loss",
    "uz_class_loss_workspace_bytes", "uz_class_loss",
    "uz_augment_params", "uz_augment_grid", "uz_augment_apply",
    "uz_patch_index_bytes", "uz_patch_index", "uz_patch_draw", "uz_patch_cut_grid", "uz_patch_cut",
    "uz_surface_workspace_bytes", "uz_surface_grid", "uz_surface_metrics",
    "uz_confusion_workspace_bytes", "uz_confusion_grid", "uz_confusion_metrics",
    "uz_boundary_workspace_bytes", "uz_boundary_grid", "uz_boundary_loss",
    "uz_lovasz_workspace_bytes", "uz_lovasz_grid", "uz_lovasz_loss",
    "uz_cldice_workspace_bytes", "uz_cldice_grid", "uz_cldice_loss",
    "uz_hardpixel_workspace_bytes", "uz_hardpixel_grid", "uz_hardpixel_loss",
    "uz_postproc_workspace_bytes", "uz_postproc_grid", "uz_postproc",
    "uz_tta_num_views", "uz_flip_views", "uz_tta_merge", "uz_mask_decide",
    "uz_tile_plan", "uz_tile_gather", "uz_tile_blend",
)


class ConvDesc(Structure):
    _fields_ = [(n, c_int) for n in (
        "dtype", "N", "H", "W", "Hin", "Win", "Cin", "ldx", "Nout", "ldy", "ntaps", "taps_mode",
        "dil", "store_mode", "Co", "Hout", "Wout")]


class WgradDesc(Structure):
    _fields_ = [(n, c_int) for n in (
        "dtype", "N", "H", "W", "Hr", "Wr", "Ci", "ldl", "Cj", "ldr", "ntaps", "taps_mode", "dil")]


class Conv5Desc(Structure):
    """uz_conv5x5_desc"""
    _fields_ = [(n, c_int) for n in ("dtype", "N", "H", "W", "Cin", "ldx", "Nout", "ldy", "ksize")]


class Wgrad5Desc(Structure):
    """uz_wgrad5x5_desc"""
    _fields_ = [(n, c_int) for n in ("dtype", "N", "H", "W", "Ci", "ldl", "Cj", "ldr", "ksize", "CiOut", "CjOut")]


class BnEluBwdDesc(Structure):
    """uz_bn_elu_bwd_desc"""
    _fields_ = [(n, c_int) for n in ("dtype", "N", "HW", "C", "ldx", "ldo", "ldg0", "ldg1", "ldg2", "lddx", "ldgres", "flags")]


class BnBwdDesc(Structure):
    _fields_ = [(n, c_int) for n in (
        "dtype", "N", "H", "W", "C", "ldy", "ldg0", "ldg1", "ldgp", "lddy", "pool_ceil")]


class LnDesc(Structure):
    _fields_ = [(n, c_int) for n in ("dtype", "N", "Ho", "Wo", "C", "ldx", "ldy", "ldr", "ldg", "lddx", "mode", "r")] \
        + [("eps", c_float), ("act", c_int)]


class WinAttnDesc(Structure):
    _fields_ = [(n, c_int) for n in ("dtype", "B", "H", "W", "C", "heads", "ws", "shift", "Nt", "ldq", "ldo")] \
        + [("scale", c_float)]


class SraDesc(Structure):
    _fields_ = [(n, c_int) for n in ("dtype", "B", "N", "NK", "heads", "head_dim", "kps", "ldq", "ldk", "ldv", "ldo")] \
        + [("scale", c_float)]


class GemmDesc(Structure):
    _fields_ = [(n, c_int) for n in ("dtype", "batch", "M", "N", "K", "ldx", "ldw", "ldy", "ldres")] \
        + [(n, ctypes.c_longlong) for n in ("xb", "wb", "yb", "resb")] + [("batch2", c_int)] \
        + [(n, ctypes.c_longlong) for n in ("xb2", "wb2", "yb2", "resb2")]


class WgradItem(Structure):
    _fields_ = [("desc", WgradDesc), ("L", c_void_p), ("R", c_void_p), ("out", c_void_p)]


class SumRowsItem(Structure):
    _fields_ = [("partial", c_void_p), ("out0", c_void_p), ("out1", c_void_p), ("rows", c_int), ("n", c_int), ("n0", c_int),
                ("reserved", c_int)]


class ColsumItem(Structure):
    _fields_ = [("x", c_void_p), ("out", c_void_p), ("P", c_int), ("C", c_int), ("ld", c_int), ("reserved", c_int)]


LN_PLAIN, LN_MERGE, LN_EXPAND = 0, 1, 2


class CpbItem(Structure):
    """uz_cpb_item: one continuous-position-bias MLP of a batched launch"""
    _fields_ = [(n, c_void_p) for n in ("idx", "w1", "b1", "w2", "b2")] \
        + [(n, c_int) for n in ("R", "hidden", "heads", "reserved")] \
        + [(n, c_void_p) for n in ("bias", "G", "dw1", "db1", "dw2", "db2")]


class PackItem(Structure):
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("begin", ctypes.c_longlong), ("mode", c_int),
                ("Co", c_int), ("Ci", c_int), ("T", c_int), ("Kpad", c_int), ("pad_", c_int)]


class Pack3x3Item(Structure):
    _fields_ = [("src", c_void_p), ("dst_fwd", c_void_p), ("dst_dgrad", c_void_p), ("Co", c_int), ("Ci", c_int),
                ("tile_begin", c_int), ("pad_", c_int)]


REGION_MAX_ITEMS = 64


class RegionItem(Structure):
    """uz_region_item: one output map of a uz_region_loss call"""
    _fields_ = [("logits", c_void_p), ("target", c_void_p), ("dlogits", c_void_p), ("weight", c_float)]


class RegionDesc(Structure):
    """uz_region_desc"""
    _fields_ = [("n_items", c_int), ("n", ctypes.c_longlong), ("groups", c_int)] \
        + [(n, c_float) for n in ("w_bce", "w_region", "alpha", "beta", "smooth", "gamma", "pos_weight")] \
        + [("metric_item", c_int)]


CLASS_MAX_ITEMS = 16
CLASS_MAX_K = 32
CLASS_REDUCE_BATCH, CLASS_REDUCE_IMAGE = 0, 1


class MapItem(Structure):
    """uz_map_item: one output map of a composed loss call; uz_class_item, uz_boundary_item, uz_lovasz_item,
    uz_cldice_item and uz_hardpixel_item are this one type"""
    _fields_ = [("logits", c_void_p), ("dlogits", c_void_p), ("weight", c_float)]


ClassItem = BoundaryItem = LovaszItem = ClDiceItem = HardPixelItem = MapItem


class ClassDesc(Structure):
    """uz_class_desc"""
    _fields_ = [("n_items", c_int), ("N", c_int), ("K", c_int), ("HW", ctypes.c_longlong)] \
        + [(n, c_float) for n in ("w_ce", "w_dice", "smooth", "label_smoothing")] \
        + [(n, c_int) for n in ("ignore_index", "reduce", "include_background", "square", "metric_item")]


AUGMENT_MASK_NONE, AUGMENT_MASK_F32, AUGMENT_MASK_I32 = 0, 1, 2


class AugmentDesc(Structure):
    """uz_augment_desc"""
    _fields_ = [(n, c_int) for n in ("N", "C", "H", "W", "mask_kind", "Cm", "G")] \
        + [(n, c_float) for n in ("p_hflip", "p_vflip", "rotate", "scale_min", "scale_max", "translate", "brightness",
                                  "contrast", "image_fill", "mask_fill")] \
        + [("label_fill", c_int)]


PATCH_IMAGE_F32, PATCH_IMAGE_U8 = 0, 1
PATCH_MASK_NONE, PATCH_MASK_F32, PATCH_MASK_I32 = 0, 1, 2


class PatchDesc(Structure):
    """uz_patch_desc"""
    _fields_ = [(n, c_int) for n in ("M", "C", "H", "W", "image_kind", "mask_kind", "Cm", "P", "B", "h", "w", "use_indices")] \
        + [("pos", c_float), ("jitter", c_float)]


SURFACE_BINARY, SURFACE_CLASS = 0, 1
SURFACE_MAX_HW = 4096


class SurfaceDesc(Structure):
    """uz_surface_desc"""
    _fields_ = [(n, c_int) for n in ("mode", "N", "C", "H", "W", "first_class", "ignore_index", "reserved")] \
        + [("q", c_double), ("spacing", c_double)]


CONFUSION_BINARY, CONFUSION_CLASS = 0, 1
CONFUSION_MAX_HW = 4096
CONFUSION_MIN_BINS, CONFUSION_MAX_BINS = 16, 1024


class ConfusionDesc(Structure):
    """uz_confusion_desc"""
    _fields_ = [(n, c_int) for n in ("mode", "N", "C", "H", "W", "first_class", "ignore_index", "bins", "max_workgroups")] \
        + [("reserved", c_int * 3)]


BOUNDARY_BINARY, BOUNDARY_CLASS = 0, 1
BOUNDARY_MAX_HW = 4096


class BoundaryDesc(Structure):
    """uz_boundary_desc"""
    _fields_ = [(n, c_int) for n in ("mode", "n_items", "N", "C", "H", "W", "first_class", "ignore_index", "metric_item")] \
        + [("spacing", c_float)]


SCHED_CONSTANT, SCHED_COSINE, SCHED_POLY, SCHED_STEP = range(4)     # UZ_SCHED_*
TAIL_STATE = 8                                                      # floats of uz_tail_step's `state`
TAIL_T, TAIL_BASE_LR, TAIL_LR, TAIL_EMA_DECAY, TAIL_CLIP, TAIL_NORM, TAIL_BC1, TAIL_BC2 = range(8)


class TailDesc(Structure):
    """uz_tail_desc"""
    _fields_ = [("n", ctypes.c_longlong)] + [(n, c_float) for n in ("beta1", "beta2", "eps", "weight_decay", "max_norm")] \
        + [("sched", c_int)] \
        + [(n, c_float) for n in ("warmup_steps", "warmup_start", "total_steps", "min_lr", "power", "gamma", "every", "ema_decay")] \
        + [("ema_warmup", c_int), ("accumulate", c_int)]


LOVASZ_BINARY, LOVASZ_CLASS = 0, 1
LOVASZ_PRESENT, LOVASZ_ALL = 0, 1
LOVASZ_MAX_SEGMENT = 1 << 22
LOVASZ_MAX_ELEMENTS = 1 << 28


class LovaszDesc(Structure):
    """uz_lovasz_desc"""
    _fields_ = [(n, c_int) for n in ("mode", "n_items", "N", "C", "H", "W", "per_image", "classes", "ignore_index", "main_item")]


CLDICE_BINARY, CLDICE_CLASS = 0, 1
CLDICE_MAX_ITERATIONS = 10       # UZ_CLDICE_MAX_ITERATIONS
CLDICE_TILE_H, CLDICE_TILE_W = 32, 32      # UZ_CLDICE_TILE_H / _W: the tile of the forward and backward passes
CLDICE_MAX_ELEMENTS = 1 << 28


class ClDiceDesc(Structure):
    """uz_cldice_desc"""
    _fields_ = [(n, c_int) for n in ("mode", "n_items", "N", "C", "H", "W", "per_image", "include_background", "ignore_index",
                                     "iterations")] + [("smooth", c_float), ("main_item", c_int)]


HARDPIXEL_BINARY, HARDPIXEL_CLASS = 0, 1
HARDPIXEL_MAX_SEGMENT = 1 << 24
HARDPIXEL_MAX_ELEMENTS = 1 << 28
HARDPIXEL_MAX_SEGMENTS = 1 << 16     # segments of a call: output maps x images with per_image
HARDPIXEL_MIN_KEEP = 2.0 ** -126     # the smallest normal fp32: what HardPixelLoss.ohem sets `keep` to
HARDPIXEL_TILE, HARDPIXEL_MAX_ROWS = 2048, 256      # a chunk is TILE * t elements, at most MAX_ROWS chunks a segment


class HardPixelDesc(Structure):
    """uz_hardpixel_desc"""
    _fields_ = [(n, c_int) for n in ("mode", "n_items", "N", "C", "H", "W", "per_image", "ignore_index", "main_item")] \
        + [("keep", c_float), ("min_kept", c_int), ("max_prob", c_float), ("gamma", c_float), ("max_workgroups", c_int)]


POST_BINARY, POST_CLASS = 0, 1
POST_MAX_KEEP = 8
POST_MAX_HW = 4096
TTA_VIEWS = {"identity": 1, "hflip": 2, "vflip": 4, "hvflip": 8}      # bit of a view; the view order is the bit order


class PostprocDesc(Structure):
    """uz_postproc_desc"""
    _fields_ = [(n, c_int) for n in ("mode", "N", "C", "H", "W", "first_class", "connectivity", "fill_holes", "min_area",
                                     "keep_largest")] + [("thr", c_float), ("reserved", c_int)]


class TtaDesc(Structure):
    """uz_tta_desc"""
    _fields_ = [(n, c_int) for n in ("mode", "N", "C", "H", "W", "views", "dtype", "reserved")]


TILE_MAX_AXIS, TILE_MAX_COVER = 256, 8
TILE_PADS = {"constant": 0, "reflect": 1}       # UZ_TILE_PAD_ZERO, UZ_TILE_PAD_REFLECT


class TileGatherDesc(Structure):
    """uz_tile_gather_desc"""
    _fields_ = [(n, c_int) for n in ("N", "C", "H", "W", "th", "tw", "ny", "nx", "pad_mode", "t0", "tn", "reserved")]


class TileBlendDesc(Structure):
    """uz_tile_blend_desc"""
    _fields_ = [(n, c_int) for n in ("N", "C", "H", "W", "th", "tw", "ny", "nx")]


class HipLibraryError(RuntimeError):
    pass


_lib = None


def load():
    """Load the kernel library once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} not found: the HIP kernel library is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` from the repo root. "
            "unet_zoo_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.uz_abi_version.restype = c_int
    lib.uz_last_error_string.restype = c_char_p
    lib.uz_source_hash.restype = c_char_p
    lib.uz_source_hash.argtypes = []
    vp, ip, fp = c_void_p, c_int, c_float
    lib.uz_set_cu_reserve.argtypes = [c_int]
    lib.uz_clock_probe.argtypes = [c_int, vp, c_int, vp]
    lib.uz_get_cu_reserve.argtypes = []
    lib.uz_conv_igemm_grid_m.argtypes = [POINTER(ConvDesc)]
    lib.uz_conv_igemm.argtypes = [POINTER(ConvDesc), vp, vp, vp, vp, vp, vp]
    lib.uz_conv_igemm_res.argtypes = [POINTER(ConvDesc), vp, vp, vp, vp, ip, vp, vp]
    lib.uz_conv_igemm_res_ws.argtypes = [POINTER(ConvDesc), vp, vp, vp, vp, ip, vp, vp, vp]
    lib.uz_conv_igemm_workspace_bytes.argtypes = [POINTER(ConvDesc)]
    lib.uz_conv_igemm_ws_grid_m.argtypes = [POINTER(ConvDesc)]
    lib.uz_conv_igemm_ws.argtypes = [POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp]
    lib.uz_conv_igemm_bnred_supported.argtypes = [POINTER(ConvDesc)]
    lib.uz_conv_igemm_xf_supported.argtypes = [POINTER(ConvDesc)]
    lib.uz_conv_igemm_xf.argtypes = [POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_conv_igemm_bnact_supported.argtypes = [POINTER(ConvDesc)]
    lib.uz_conv_igemm_bnact.argtypes = [POINTER(ConvDesc), vp, vp, vp, vp, vp, c_int, vp, vp]
    lib.uz_conv_igemm_kernel_name.argtypes = [POINTER(ConvDesc), c_int, c_char_p, c_int]
    lib.uz_profile_arm.argtypes = [vp, vp]
    lib.uz_profile_disarm.argtypes = []
    lib.uz_conv_igemm_bnred.argtypes = [POINTER(ConvDesc), vp, vp, vp, vp, c_int, vp, vp, vp, vp, vp, vp]
    lib.uz_bn_bwd_finalize.argtypes = [vp, c_int, c_int, vp, vp, vp, vp]
    lib.uz_patchify.argtypes = [ip, vp, ip, ip, ip, ip, ip, ip, vp, vp]
    lib.uz_layernorm_fwd.argtypes = [POINTER(LnDesc), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_layernorm_act_bwd.argtypes = [POINTER(LnDesc), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_layernorm_bwd_rows.argtypes = [POINTER(LnDesc)]
    lib.uz_layernorm_bwd.argtypes = [POINTER(LnDesc), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_ln_head_fwd.argtypes = [POINTER(LnDesc), vp, vp, vp, vp, vp, ip, vp, vp, vp]
    lib.uz_ln_head_bwd_workspace_bytes.argtypes = [POINTER(LnDesc), ip]
    lib.uz_ln_head_bwd.argtypes = [POINTER(LnDesc), vp, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_sum_rows_f32_ld.argtypes = [vp, ip, ip, ip, vp, ip, vp, vp]
    lib.uz_winattn_fwd.argtypes = [POINTER(WinAttnDesc), vp, vp, vp, vp, vp, vp]
    lib.uz_winattn_bwd_rows.argtypes = [POINTER(WinAttnDesc)]
    lib.uz_winattn_bwd.argtypes = [POINTER(WinAttnDesc), vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, vp]
    lib.uz_colstats_rows.argtypes = [ip, ip, ip]
    lib.uz_colstats.argtypes = [ip, vp, ip, ip, ip, vp, vp]
    lib.uz_cpb_fwd.argtypes = [vp, vp, vp, vp, vp, ip, ip, ip, vp, vp]
    lib.uz_cpb_bwd.argtypes = [vp, vp, vp, vp, vp, ip, ip, ip, vp, vp, vp, vp, vp]
    lib.uz_cpb_fwd_batched.argtypes = [vp, ip, vp]
    lib.uz_cpb_bwd_batched_workspace_bytes.argtypes = [vp, ip]
    lib.uz_cpb_bwd_batched.argtypes = [vp, ip, vp, vp]
    lib.uz_clip_adamw_workspace_bytes.argtypes = []
    lib.uz_clip_adamw.argtypes = [vp, vp, vp, vp, ctypes.c_longlong, fp, fp, fp, fp, fp, fp, vp, vp, vp]
    lib.uz_tail_workspace_bytes.argtypes = []
    lib.uz_tail_step.argtypes = [POINTER(TailDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_tail_accumulate.argtypes = [vp, vp, ctypes.c_longlong, ip, vp]
    lib.uz_tail_swap.argtypes = [vp, vp, ctypes.c_longlong, vp]
    lib.uz_wgrad_split.argtypes = [POINTER(WgradDesc)]
    lib.uz_wgrad_workspace_bytes.argtypes = [POINTER(WgradDesc)]
    lib.uz_wgrad.argtypes = [POINTER(WgradDesc), vp, vp, vp, vp, vp]
    lib.uz_wgrad_kernel_name.argtypes = [POINTER(WgradDesc), c_char_p, c_int]
    lib.uz_wgrad_phase.argtypes = [POINTER(WgradDesc), vp, vp, vp, vp, vp, c_int]
    lib.uz_wgrad_xf_supported.argtypes = [POINTER(WgradDesc)]
    lib.uz_wgrad_xf.argtypes = [POINTER(WgradDesc), vp, vp, vp, vp, vp, vp, vp, c_int]
    lib.uz_conv3x3_first_supported.argtypes = [ip, ip, ip]
    lib.uz_conv3x3_first_rows.argtypes = [ip, ip, ip]
    lib.uz_conv3x3_first_fwd.argtypes = [ip, vp, ip, ip, ip, ip, vp, vp, ip, vp, ip, vp, vp]
    lib.uz_conv3x3_first_fwd_bnact.argtypes = [ip, vp, ip, ip, ip, ip, vp, vp, ip, vp, vp, ip, vp, ip, vp]
    lib.uz_conv3x3_first_wgrad_workspace_bytes.argtypes = [ip, ip, ip, ip]
    lib.uz_conv3x3_first_wgrad_workspace_bytes.restype = ctypes.c_longlong
    lib.uz_conv3x3_first_wgrad.argtypes = [ip, vp, ip, ip, ip, ip, vp, ip, ip, vp, vp, vp]
    lib.uz_conv3x3_first_wgrad_bn.argtypes = [ip, vp, ip, ip, ip, ip, vp, ip, vp, ip, vp, vp, vp, vp, vp, ctypes.c_double, ip, vp, vp, vp]
    lib.uz_pack_weights.argtypes = [ip, ip, vp, ip, ip, ip, ip, vp, vp]
    lib.uz_pack_weights_batched.argtypes = [ip, vp, ip, ctypes.c_longlong, vp]
    lib.uz_pack_conv3x3_batched.argtypes = [ip, vp, ip, ip, vp]
    lib.uz_im2col3x3_nchw.argtypes = [ip, vp, ip, ip, ip, ip, ip, vp, vp]
    lib.uz_bn_finalize.argtypes = [vp, ip, ip, c_double, vp, vp, fp, fp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_bn_eval_scale.argtypes = [ip, vp, vp, vp, vp, fp, vp, vp, vp]
    lib.uz_bn_relu_apply.argtypes = [ip, vp, ip, vp, vp, ip, ip, ip, ip, vp, ip, vp, ip, vp]
    lib.uz_bn_relu_bwd_workspace_bytes.argtypes = [POINTER(BnBwdDesc), ip]
    lib.uz_bn_relu_bwd_reduce.argtypes = [POINTER(BnBwdDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                          vp, vp, vp]
    lib.uz_bn_relu_bwd_apply.argtypes = [POINTER(BnBwdDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                         c_double, vp, vp]
    lib.uz_outconv_fwd.argtypes = [ip, vp, ip, ip, ip, ip, vp, vp, ip, vp, vp]
    lib.uz_outconv_fwd_xf.argtypes = [ip, vp, ip, ip, ip, ip, vp, vp, vp, vp, ip, vp, vp]
    lib.uz_outconv_bwd_workspace_bytes.argtypes = [ip, ip, ip, ip, ip]
    lib.uz_outconv_bwd.argtypes = [ip, vp, ip, ip, ip, ip, vp, ip, vp, vp, ip, vp, vp, vp, vp]
    lib.uz_outconv_bwd_rows.argtypes = [ip, ip, ip, ip]
    lib.uz_head_wide_supported.argtypes = [ip, ip, ip]
    lib.uz_head_wide_grid.argtypes = [ip, ip, ip, ip, ip]
    lib.uz_head_wide_fwd.argtypes = [ip, vp, ip, ip, ip, ip, vp, vp, ip, vp, vp]
    lib.uz_head_wide_bwd_workspace_bytes.argtypes = [ip, ip, ip, ip, ip]
    lib.uz_head_wide_bwd.argtypes = [ip, vp, ip, ip, ip, ip, vp, ip, vp, vp, ip, vp, vp, vp, vp]
    lib.uz_bn_relu_bwd_apply_head_supported.argtypes = [ip, ip, ip]
    lib.uz_bn_relu_bwd_apply_head.argtypes = [POINTER(BnBwdDesc), vp, vp, vp, vp, vp, vp, vp, ip, vp, ctypes.c_double, vp, vp]
    lib.uz_outconv_bwd_bnred.argtypes = [ip, vp, ip, ip, ip, ip, vp, ip, vp, vp, ip, vp, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp]
    lib.uz_colsum.argtypes = [ip, vp, ip, ip, ip, vp, vp]
    lib.uz_colsum_workspace_bytes.argtypes = [ip, ip, ip]
    lib.uz_colsum_ws.argtypes = [ip, vp, ip, ip, ip, vp, vp, vp]
    lib.uz_attn_grid.argtypes = [ip, ip, ip]
    lib.uz_attn_psi_fwd.argtypes = [ip, vp, ip, vp, ip, vp, vp, vp, vp, ip, ip, vp, vp, vp]
    lib.uz_attn_gate_fwd.argtypes = [ip, vp, ip, vp, vp, ip, ip, vp, ip, vp]
    lib.uz_attn_bwd_psi.argtypes = [ip, vp, ip, vp, ip, vp, vp, ip, ip, vp, ip, vp, vp, vp]
    lib.uz_attn_bwd_reduce.argtypes = [ip, vp, ip, vp, ip, vp, vp, vp, vp, vp, vp, vp, ip, ip, vp, vp]
    lib.uz_attn_bwd_apply.argtypes = [ip, vp, ip, vp, ip, vp, vp, vp, vp, vp, vp, vp, vp, ip, ip, vp, ip,
                                      vp, ip, vp]
    lib.uz_sum_rows.argtypes = [vp, ip, ip, vp, vp]
    lib.uz_sum_rows_f32.argtypes = [vp, ip, ip, vp, ip, vp, vp]
    lib.uz_sum2x2.argtypes = [ip, vp, ip, ip, ip, ip, ip, vp, ip, vp]
    ll = ctypes.c_longlong
    lib.uz_bn_relu_add_apply.argtypes = [ip, vp, ip, vp, vp, ip, ip, ip, ip, vp, ip, vp, ip, vp, ip, ip, vp]
    lib.uz_bn_relu_add_apply_fin.argtypes = [ip, vp, ip, vp, ip, ctypes.c_double, vp, vp, c_float, c_float, vp, vp, vp, vp,
                                             ip, ip, ip, ip, vp, ip, vp, ip, vp, ip, ip, vp]
    lib.uz_bn_relu_bwd_reduce_rows.argtypes = [POINTER(BnBwdDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_bn_relu_bwd_apply_fin.argtypes = [POINTER(BnBwdDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, ip, vp, vp, vp, vp,
                                             ctypes.c_double, vp, vp]
    lib.uz_bilinear_fwd.argtypes = [ip, vp, ip, ll, ip, ip, ip, ip, vp, ip, ll, ip, ip, vp]
    lib.uz_bilinear_bwd.argtypes = [ip, vp, ip, ll, ip, ip, ip, ip, vp, ip, ll, ip, ip, vp]
    lib.uz_resize_bilinear_fwd.argtypes = [ip, vp, ip, ll, ip, ip, ip, ip, vp, ip, ll, ip, ip, ip, vp]
    lib.uz_resize_bilinear_bwd.argtypes = [ip, vp, ip, ll, ip, ip, ip, ip, vp, ip, ll, ip, ip, ip, vp]
    lib.uz_resample2.argtypes = [ip, vp, ip, ip, ip, ip, ip, vp, ip, ip, ip, ip, vp]
    lib.uz_pool_grad_combine.argtypes = [ip, ip, ip, ip, ip, vp, ip, vp, ip, vp, ip, vp, ip, vp, ip, ip, vp]
    lib.uz_sideconv3x3_fwd.argtypes = [ip, vp, ip, ip, ip, ip, ip, vp, vp, vp, vp, ll, vp]
    lib.uz_sideconv3x3_bwd_workspace_bytes.argtypes = [ip, ip, ip, ip, ip]
    lib.uz_sideconv3x3_bwd.argtypes = [ip, vp, ip, ip, ip, ip, ip, vp, vp, ll, vp, ip, vp, vp, vp, vp]
    lib.uz_fuse1x1_fwd.argtypes = [vp, ip, ip, ip, ip, vp, vp, vp, vp]
    lib.uz_fuse1x1_bwd_workspace_bytes.argtypes = [ip, ip, ip, ip]
    lib.uz_fuse1x1_bwd.argtypes = [vp, ip, ip, ip, ip, vp, vp, POINTER(c_void_p), ip, vp, vp, vp, vp, vp]
    lib.uz_sum_rows_f32_batched.argtypes = [POINTER(SumRowsItem), ip, vp]
    lib.uz_wgrad_multi_workspace_bytes.argtypes = [POINTER(WgradItem), ip]
    lib.uz_wgrad_multi_workspace_bytes.restype = ctypes.c_longlong
    lib.uz_wgrad_multi.argtypes = [POINTER(WgradItem), ip, vp, vp]
    lib.uz_colsum_batched_workspace_bytes.argtypes = [ip, POINTER(ColsumItem), ip]
    lib.uz_colsum_batched.argtypes = [ip, POINTER(ColsumItem), ip, vp, vp]
    lib.uz_bce_dice_workspace_bytes.argtypes = [ll]
    lib.uz_bce_dice.argtypes = [vp, vp, ll, vp, vp, vp, vp]
    lib.uz_gelu_fwd.argtypes = [ip, vp, ip, vp, ip, ll, ip, vp]
    lib.uz_gelu_bwd.argtypes = [ip, vp, ip, vp, ip, vp, ip, ll, ip, vp]
    lib.uz_dwconv3x3.argtypes = [ip, vp, ip, vp, vp, vp, ip, ip, ip, ip, ip, ip, vp]
    lib.uz_dwconv3x3_wgrad_rows.argtypes = [ip, ip, ip, ip, ip]
    lib.uz_dwconv3x3_wgrad.argtypes = [ip, vp, ip, vp, ip, vp, ip, ip, ip, ip, vp]
    lib.uz_space_to_depth.argtypes = [ip, vp, ip, vp, ip, ip, ip, ip, ip, ip, ip, vp]
    lib.uz_space_to_depth_crop.argtypes = [ip, vp, ip, vp, ip, ip, ip, ip, ip, ip, ip, vp]
    lib.uz_im2col_nchw.argtypes = [ip, vp, ip, ip, ip, ip, ip, ip, ip, ip, vp, vp]
    lib.uz_sra_fwd.argtypes = [POINTER(SraDesc), vp, vp, vp, vp, vp, vp]
    lib.uz_sra_bwd_workspace_bytes.argtypes = [POINTER(SraDesc)]
    lib.uz_sra_bwd.argtypes = [POINTER(SraDesc), vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, ip, vp, vp]
    lib.uz_add_relu.argtypes = [ip, vp, ip, vp, ip, vp, ip, ll, ip, vp]
    lib.uz_relu_bwd.argtypes = [ip, vp, ip, vp, ip, vp, ip, ll, ip, vp]
    lib.uz_pil_resample_h_u8.argtypes = [vp, ip, ip, ip, vp, vp, ip, ip, vp, vp]
    lib.uz_pil_resample_v_f32.argtypes = [vp, ip, ip, ip, vp, vp, ip, ip, POINTER(c_float), POINTER(c_float), ip, vp, vp]
    lib.uz_wgrad_batched_workspace_bytes.argtypes = [POINTER(WgradDesc), ip]
    lib.uz_wgrad_batched.argtypes = [POINTER(WgradDesc), ip, vp, ll, vp, ll, vp, ll, vp, vp]
    lib.uz_wgrad_batched2.argtypes = [POINTER(WgradDesc), ip, ip, vp, ll, ll, vp, ll, ll, vp, ll, vp, vp]
    lib.uz_gemm_nt.argtypes = [POINTER(GemmDesc), vp, vp, vp, vp, vp, vp]
    lib.uz_softmax_workspace_bytes.argtypes = [ip, ip, ip, ip]
    lib.uz_softmax_fwd.argtypes = [ip, vp, ip, ll, ip, ip, ip, ip, c_float, vp, vp]
    lib.uz_chanattn_probs_fwd.argtypes = [ip, vp, ip, ip, ip, ip, c_float, c_float, vp, vp, vp]
    lib.uz_chanattn_probs_bwd.argtypes = [ip, vp, vp, ip, ip, ip, ip, c_float, c_float, vp, vp, vp]
    lib.uz_dropout.argtypes = [ip, vp, ip, vp, c_float, vp, ip, ll, ip, vp]
    lib.uz_chanscale_relu.argtypes = [ip, ip, vp, ip, vp, ip, vp, vp, ip, ip, ip, vp, ip, vp]
    lib.uz_add_map.argtypes = [ip, vp, ip, vp, vp, ip, ll, ip, ip, vp]
    lib.uz_softmax_bwd.argtypes = [ip, vp, vp, ip, ll, ip, ip, ip, ip, c_float, vp, ip, vp]
    lib.uz_adaptive_avgpool_fwd.argtypes = [ip, vp, ip, ip, ip, ip, ip, vp, ip, ip, ip, vp]
    lib.uz_adaptive_avgpool_bwd.argtypes = [ip, vp, ip, ip, ip, ip, ip, vp, ip, ip, ip, ip, vp]
    lib.uz_rowdot_f32.argtypes = [ip, vp, ip, vp, ip, ll, ip, vp, vp]
    lib.uz_cast_rows.argtypes = [ip, vp, ip, vp, ip, ll, ip, ip, vp]
    lib.uz_conv5x5_grid_m.argtypes = [POINTER(Conv5Desc)]
    lib.uz_conv5x5.argtypes = [POINTER(Conv5Desc), vp, vp, vp, vp, vp, vp]
    lib.uz_wgrad5x5_workspace_bytes.argtypes = [POINTER(Wgrad5Desc)]
    lib.uz_wgrad5x5.argtypes = [POINTER(Wgrad5Desc), vp, vp, vp, vp, vp]
    lib.uz_bn_elu_apply.argtypes = [ip, vp, ip, vp, vp, ip, ip, ip, vp, ip, vp, ip, vp, ip, vp, ip, vp]
    lib.uz_bn_elu_bwd_rows.argtypes = [POINTER(BnEluBwdDesc)]
    lib.uz_bn_elu_bwd_reduce.argtypes = [POINTER(BnEluBwdDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_bn_elu_bwd_apply.argtypes = [POINTER(BnEluBwdDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_region_loss_workspace_bytes.argtypes = [POINTER(RegionDesc)]
    lib.uz_region_loss.argtypes = [POINTER(RegionDesc), POINTER(RegionItem), vp, vp, vp]
    lib.uz_class_loss_workspace_bytes.argtypes = [POINTER(ClassDesc)]
    lib.uz_class_loss.argtypes = [POINTER(ClassDesc), POINTER(ClassItem), vp, vp, vp, vp, vp, vp]
    lib.uz_augment_params.argtypes = [POINTER(AugmentDesc), vp, vp, vp]
    lib.uz_augment_grid.argtypes = [POINTER(AugmentDesc), POINTER(c_int)]
    lib.uz_augment_apply.argtypes = [POINTER(AugmentDesc), vp, vp, vp, vp, vp, vp, vp]
    lib.uz_patch_index_bytes.argtypes = [POINTER(PatchDesc)]
    lib.uz_patch_index.argtypes = [POINTER(PatchDesc), vp, vp, vp]
    lib.uz_patch_draw.argtypes = [POINTER(PatchDesc), vp, vp, vp, vp, vp, vp]
    lib.uz_patch_cut_grid.argtypes = [POINTER(PatchDesc), POINTER(c_int)]
    lib.uz_patch_cut.argtypes = [POINTER(PatchDesc), vp, vp, vp, vp, vp, vp, vp]
    lib.uz_surface_workspace_bytes.argtypes = [POINTER(SurfaceDesc)]
    lib.uz_surface_grid.argtypes = [POINTER(SurfaceDesc), POINTER(c_int)]
    lib.uz_surface_metrics.argtypes = [POINTER(SurfaceDesc), vp, vp, vp, vp, vp, vp]
    lib.uz_confusion_workspace_bytes.argtypes = [POINTER(ConfusionDesc)]
    lib.uz_confusion_grid.argtypes = [POINTER(ConfusionDesc), POINTER(c_int)]
    lib.uz_confusion_metrics.argtypes = [POINTER(ConfusionDesc), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_boundary_workspace_bytes.argtypes = [POINTER(BoundaryDesc)]
    lib.uz_boundary_grid.argtypes = [POINTER(BoundaryDesc), POINTER(c_int)]
    lib.uz_boundary_loss.argtypes = [POINTER(BoundaryDesc), POINTER(BoundaryItem), vp, vp, vp, vp, vp, vp, vp]
    lib.uz_lovasz_workspace_bytes.argtypes = [POINTER(LovaszDesc)]
    lib.uz_lovasz_grid.argtypes = [POINTER(LovaszDesc), POINTER(c_int)]
    lib.uz_lovasz_loss.argtypes = [POINTER(LovaszDesc), POINTER(LovaszItem), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_cldice_workspace_bytes.argtypes = [POINTER(ClDiceDesc)]
    lib.uz_cldice_grid.argtypes = [POINTER(ClDiceDesc), POINTER(c_int)]
    lib.uz_cldice_loss.argtypes = [POINTER(ClDiceDesc), POINTER(ClDiceItem), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_hardpixel_workspace_bytes.argtypes = [POINTER(HardPixelDesc)]
    lib.uz_hardpixel_grid.argtypes = [POINTER(HardPixelDesc), POINTER(c_int)]
    lib.uz_hardpixel_loss.argtypes = [POINTER(HardPixelDesc), POINTER(HardPixelItem), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_postproc_workspace_bytes.argtypes = [POINTER(PostprocDesc)]
    lib.uz_postproc_grid.argtypes = [POINTER(PostprocDesc), POINTER(c_int)]
    lib.uz_postproc.argtypes = [POINTER(PostprocDesc), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uz_tta_num_views.argtypes = [c_int]
    lib.uz_flip_views.argtypes = [POINTER(TtaDesc), vp, POINTER(c_void_p), vp]
    lib.uz_tta_merge.argtypes = [POINTER(TtaDesc), POINTER(c_void_p), vp, vp]
    lib.uz_mask_decide.argtypes = [POINTER(TtaDesc), vp, c_float, c_int, vp, vp, vp]
    lib.uz_tile_plan.argtypes = [c_int, c_int, c_double, POINTER(c_int), c_int]
    lib.uz_tile_gather.argtypes = [POINTER(TileGatherDesc), POINTER(c_int), POINTER(c_int), vp, vp, vp]
    lib.uz_tile_blend.argtypes = [POINTER(TileBlendDesc), POINTER(c_int), POINTER(c_int), vp, vp, vp, vp, vp]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("uz_last_error_string", "uz_source_hash"):
            fn.restype = ctypes.c_longlong if name.endswith(("_workspace_bytes", "_index_bytes")) else c_int
    if lib.uz_abi_version() != 1:
        raise HipLibraryError("libunetzoo_hip.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib


def _fail(rc: int, what: str):
    msg = load().uz_last_error_string().decode("utf-8", "replace")
    raise HipLibraryError(f"{what} failed (code {rc}): {msg}")


def check(rc: int, what: str) -> None:
    """Status-returning entry points: anything but 0 is an error."""
    if rc != 0:
        _fail(rc, what)


def check_count(rc: int, what: str) -> int:
    """Count-returning entry points (grid_m, split): negative is an error."""
    if rc < 0:
        _fail(rc, what)
    return rc


def _desc_bytes(name: str, desc) -> int:
    """A byte count of a descriptor (uz_X_workspace_bytes, uz_patch_index_bytes): negative is the library's refusal."""
    return check_count(getattr(load(), name)(ctypes.byref(desc)), name)


def _desc_grid(name: str, desc) -> tuple:
    """(workgroups, units) of a descriptor (uz_X_grid): units > workgroups means workgroups walk."""
    units = c_int(0)
    grid = check_count(getattr(load(), name)(ctypes.byref(desc), ctypes.byref(units)), name)
    return grid, units.value


def region_loss_workspace_bytes(desc: "RegionDesc") -> int:
    """uz_region_loss_workspace_bytes(): bytes of workspace a uz_region_loss call with this descriptor needs"""
    return _desc_bytes("uz_region_loss_workspace_bytes", desc)


def region_loss(desc: "RegionDesc", items, out2: torch.Tensor, workspace: torch.Tensor) -> None:
    """uz_region_loss() on the current stream: `items` is a ctypes array of RegionItem (a HOST table, copied into the
    kernel arguments), out2 a 2-element fp32 device tensor (loss, dice).  Every call of the loss goes through here."""
    check(load().uz_region_loss(ctypes.byref(desc), items, out2.data_ptr(), workspace.data_ptr(), stream_ptr()),
          "uz_region_loss")


def class_loss_workspace_bytes(desc: "ClassDesc") -> int:
    """uz_class_loss_workspace_bytes(): bytes of workspace a uz_class_loss call with this descriptor needs"""
    return _desc_bytes("uz_class_loss_workspace_bytes", desc)


def class_loss(desc: "ClassDesc", items, labels: torch.Tensor, class_weight, out2: torch.Tensor, counts: torch.Tensor,
               workspace: torch.Tensor) -> None:
    """uz_class_loss() on the current stream: `items` is a ctypes array of ClassItem (a HOST table, copied into the kernel
    arguments), labels an int32 (N, HW) device tensor, class_weight K fp32 on the device or None, out2 a 2-element fp32
    device tensor (loss, dice), counts a (K + 1, 3) int64 device tensor.  Every call of the loss goes through here."""
    check(load().uz_class_loss(ctypes.byref(desc), items, labels.data_ptr(),
                               class_weight.data_ptr() if class_weight is not None else None, out2.data_ptr(),
                               counts.data_ptr() if counts is not None else None, workspace.data_ptr(), stream_ptr()),
          "uz_class_loss")


def surface_workspace_bytes(desc: "SurfaceDesc") -> int:
    """uz_surface_workspace_bytes(): bytes of workspace a uz_surface_metrics call with this descriptor needs"""
    return _desc_bytes("uz_surface_workspace_bytes", desc)


def surface_grid(desc: "SurfaceDesc") -> tuple:
    """uz_surface_grid(): (workgroups, units) of the widest launch of uz_surface_metrics for this descriptor"""
    return _desc_grid("uz_surface_grid", desc)


def surface_metrics(desc: "SurfaceDesc", logits: torch.Tensor, target: torch.Tensor, out: torch.Tensor, stats: torch.Tensor,
                    workspace: torch.Tensor) -> None:
    """uz_surface_metrics() on the current stream: seven launches, no allocation, no host read"""
    check(load().uz_surface_metrics(ctypes.byref(desc), logits.data_ptr(), target.data_ptr(), out.data_ptr(), stats.data_ptr(),
                                    workspace.data_ptr(), stream_ptr()), "uz_surface_metrics")


def confusion_workspace_bytes(desc: "ConfusionDesc") -> int:
    """uz_confusion_workspace_bytes(): bytes of workspace a uz_confusion_metrics call with this descriptor needs"""
    return _desc_bytes("uz_confusion_workspace_bytes", desc)


def confusion_grid(desc: "ConfusionDesc") -> tuple:
    """uz_confusion_grid(): (workgroups, units) of the counting pass of uz_confusion_metrics for this descriptor"""
    return _desc_grid("uz_confusion_grid", desc)


def confusion_metrics(desc: "ConfusionDesc", logits: torch.Tensor, target: torch.Tensor, edges, counts: torch.Tensor, hist,
                      out: torch.Tensor, workspace: torch.Tensor) -> None:
    """uz_confusion_metrics() on the current stream: three launches, no allocation, no host read; edges and hist are None in
    the class mode"""
    check(load().uz_confusion_metrics(ctypes.byref(desc), logits.data_ptr(), target.data_ptr(),
                                      edges.data_ptr() if edges is not None else None, counts.data_ptr(),
                                      hist.data_ptr() if hist is not None else None, out.data_ptr(), workspace.data_ptr(),
                                      stream_ptr()), "uz_confusion_metrics")


def boundary_workspace_bytes(desc: "BoundaryDesc") -> int:
    """uz_boundary_workspace_bytes(): bytes of workspace a uz_boundary_loss call with this descriptor needs"""
    return _desc_bytes("uz_boundary_workspace_bytes", desc)


def boundary_grid(desc: "BoundaryDesc") -> tuple:
    """uz_boundary_grid(): (workgroups, units) of the column pass of uz_boundary_loss for this descriptor"""
    return _desc_grid("uz_boundary_grid", desc)


def boundary_loss(desc: "BoundaryDesc", items, target: torch.Tensor, scales: torch.Tensor, base_loss: torch.Tensor,
                  out2: torch.Tensor, sd2: torch.Tensor, workspace: torch.Tensor) -> None:
    """uz_boundary_loss() on the current stream: `items` is a ctypes array of BoundaryItem (a HOST table, copied into the
    kernel arguments), scales the (weight, base_scale) pair and base_loss the base criterion's value ON THE DEVICE, out2 a
    2-element fp32 device tensor (loss, boundary term of the main map), sd2 the int32 (M, H, W) transform it writes.  Five
    launches, no allocation, no host read.  Every call of the loss goes through here."""
    check(load().uz_boundary_loss(ctypes.byref(desc), items, target.data_ptr(), scales.data_ptr(), base_loss.data_ptr(),
                                  out2.data_ptr(), sd2.data_ptr(), workspace.data_ptr(), stream_ptr()), "uz_boundary_loss")


def lovasz_workspace_bytes(desc: "LovaszDesc") -> int:
    """uz_lovasz_workspace_bytes(): bytes of workspace a uz_lovasz_loss call with this descriptor needs"""
    return _desc_bytes("uz_lovasz_workspace_bytes", desc)


def lovasz_grid(desc: "LovaszDesc") -> tuple:
    """uz_lovasz_grid(): (workgroups, units) of the passes over (segment, tile) units of uz_lovasz_loss for this descriptor"""
    return _desc_grid("uz_lovasz_grid", desc)


def lovasz_loss(desc: "LovaszDesc", items, target: torch.Tensor, scales: torch.Tensor, base_loss: torch.Tensor,
                out2: torch.Tensor, errors: torch.Tensor, ranks: torch.Tensor, workspace: torch.Tensor) -> None:
    """uz_lovasz_loss() on the current stream: `items` is a ctypes array of LovaszItem (a HOST table, copied into the kernel
    arguments), scales the (weight, base_scale) pair and base_loss the base criterion's value ON THE DEVICE, out2 a 2-element
    fp32 device tensor (loss, V of the main map), errors (fp32) and ranks (int32) the (segments, length) outputs of the main
    map.  18 or 19 launches, no allocation, no host read.  Every call of the loss goes through here."""
    check(load().uz_lovasz_loss(ctypes.byref(desc), items, target.data_ptr(), scales.data_ptr(), base_loss.data_ptr(),
                                out2.data_ptr(), errors.data_ptr(), ranks.data_ptr(), workspace.data_ptr(), stream_ptr()),
          "uz_lovasz_loss")


def cldice_workspace_bytes(desc: "ClDiceDesc") -> int:
    """uz_cldice_workspace_bytes(): bytes of workspace a uz_cldice_loss call with this descriptor needs"""
    return _desc_bytes("uz_cldice_workspace_bytes", desc)


def cldice_grid(desc: "ClDiceDesc") -> tuple:
    """uz_cldice_grid(): (workgroups, units) of the passes over (map, plane, tile) units of uz_cldice_loss for this descriptor"""
    return _desc_grid("uz_cldice_grid", desc)


def cldice_loss(desc: "ClDiceDesc", items, target: torch.Tensor, scales: torch.Tensor, base_loss: torch.Tensor,
                out2: torch.Tensor, probs: torch.Tensor, skeleton: torch.Tensor, target_skeleton: torch.Tensor,
                workspace: torch.Tensor) -> None:
    """uz_cldice_loss() on the current stream: `items` is a ctypes array of ClDiceItem (a HOST table, copied into the kernel
    arguments), scales the (weight, base_scale) pair and base_loss the base criterion's value ON THE DEVICE, out2 a 2-element
    fp32 device tensor (loss, V of the main map), probs / skeleton the (N, C, H, W) fp32 planes of the main map and
    target_skeleton the target's.  4 or 6 launches, no allocation, no host read.  Every call of the loss goes through here."""
    check(load().uz_cldice_loss(ctypes.byref(desc), items, target.data_ptr(), scales.data_ptr(), base_loss.data_ptr(),
                                out2.data_ptr(), probs.data_ptr(), skeleton.data_ptr(), target_skeleton.data_ptr(),
                                workspace.data_ptr(), stream_ptr()), "uz_cldice_loss")


def hardpixel_workspace_bytes(desc: "HardPixelDesc") -> int:
    """uz_hardpixel_workspace_bytes(): bytes of workspace a uz_hardpixel_loss call with this descriptor needs"""
    return _desc_bytes("uz_hardpixel_workspace_bytes", desc)


def hardpixel_grid(desc: "HardPixelDesc") -> tuple:
    """uz_hardpixel_grid(): (workgroups, units) of the passes over (segment, chunk) units of uz_hardpixel_loss for this
    descriptor"""
    return _desc_grid("uz_hardpixel_grid", desc)


def hardpixel_loss(desc: "HardPixelDesc", items, target: torch.Tensor, scales: torch.Tensor, base_loss: torch.Tensor,
                   out2: torch.Tensor, losses: torch.Tensor, selection: torch.Tensor, workspace: torch.Tensor) -> None:
    """uz_hardpixel_loss() on the current stream: `items` is a ctypes array of HardPixelItem (a HOST table, copied into the
    kernel arguments), scales the (weight, base_scale) pair and base_loss the base criterion's value ON THE DEVICE, out2 a
    2-element fp32 device tensor (loss, V of the main map), losses (fp32, the map's layout) and selection (int32,
    (segments, 4)) the outputs of the main map.  10 launches, no allocation, no host read.  Every call of the loss goes
    through here."""
    check(load().uz_hardpixel_loss(ctypes.byref(desc), items, target.data_ptr(), scales.data_ptr(), base_loss.data_ptr(),
                                   out2.data_ptr(), losses.data_ptr(), selection.data_ptr(), workspace.data_ptr(), stream_ptr()),
          "uz_hardpixel_loss")


def postproc_workspace_bytes(desc: "PostprocDesc") -> int:
    """uz_postproc_workspace_bytes(): bytes of workspace a uz_postproc call with this descriptor needs"""
    return _desc_bytes("uz_postproc_workspace_bytes", desc)


def postproc_grid(desc: "PostprocDesc") -> tuple:
    """uz_postproc_grid(): (workgroups, units) of the per-unit launches of uz_postproc for this descriptor"""
    return _desc_grid("uz_postproc_grid", desc)


def _ptr(t) -> "int | None":
    return t.data_ptr() if t is not None else None


def postproc(desc: "PostprocDesc", x: torch.Tensor, mask: torch.Tensor, labels, class_map, stats: torch.Tensor, comps: torch.Tensor,
             workspace: torch.Tensor) -> None:
    """uz_postproc() on the current stream: a fixed number of launches, no allocation, no host read"""
    check(load().uz_postproc(ctypes.byref(desc), x.data_ptr(), mask.data_ptr(), _ptr(labels), _ptr(class_map), stats.data_ptr(),
                             comps.data_ptr(), workspace.data_ptr(), stream_ptr()), "uz_postproc")


def _ptr_table(tensors):
    return (c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def flip_views(desc: "TtaDesc", x: torch.Tensor, views) -> None:
    """uz_flip_views() on the current stream: one launch (`views`: the V output tensors; a HOST pointer table)"""
    check(load().uz_flip_views(ctypes.byref(desc), x.data_ptr(), _ptr_table(views), stream_ptr()), "uz_flip_views")


def tta_merge(desc: "TtaDesc", logits, prob: torch.Tensor) -> None:
    """uz_tta_merge() on the current stream: one launch (`logits`: the V tensors in view order)"""
    check(load().uz_tta_merge(ctypes.byref(desc), _ptr_table(logits), prob.data_ptr(), stream_ptr()), "uz_tta_merge")


def mask_decide(desc: "TtaDesc", x: torch.Tensor, thr: float, first_class: int, mask: torch.Tensor, class_map) -> None:
    """uz_mask_decide() on the current stream: one launch"""
    check(load().uz_mask_decide(ctypes.byref(desc), x.data_ptr(), float(thr), int(first_class), mask.data_ptr(), _ptr(class_map),
                                stream_ptr()), "uz_mask_decide")


def tile_plan(size: int, window: int, overlap: float) -> list:
    """uz_tile_plan(): the tile starts along one axis (host code; no GPU call)"""
    starts = (c_int * TILE_MAX_AXIS)()
    n = check_count(load().uz_tile_plan(int(size), int(window), float(overlap), starts, TILE_MAX_AXIS), "uz_tile_plan")
    return [int(starts[i]) for i in range(n)]


def _int_table(values):
    return (c_int * len(values))(*[int(v) for v in values])


def tile_gather(desc: "TileGatherDesc", ys, xs, x: torch.Tensor, out: torch.Tensor) -> None:
    """uz_tile_gather() on the current stream: one launch (`ys`, `xs`: HOST start tables, copied into the kernel arguments)"""
    check(load().uz_tile_gather(ctypes.byref(desc), _int_table(ys), _int_table(xs), x.data_ptr(), out.data_ptr(), stream_ptr()),
          "uz_tile_gather")


def tile_blend(desc: "TileBlendDesc", ys, xs, tiles: torch.Tensor, gh: torch.Tensor, gw: torch.Tensor, out: torch.Tensor) -> None:
    """uz_tile_blend() on the current stream: one launch (`gh`, `gw`: DEVICE weight tables)"""
    check(load().uz_tile_blend(ctypes.byref(desc), _int_table(ys), _int_table(xs), tiles.data_ptr(), gh.data_ptr(), gw.data_ptr(),
                               out.data_ptr(), stream_ptr()), "uz_tile_blend")


def set_cu_reserve(n: int) -> None:
    """uz_set_cu_reserve(): size every persistent grid of the library for 256 - n CUs (process-wide; call before any
    plan is queried / any graph is captured)"""
    check(load().uz_set_cu_reserve(int(n)), "uz_set_cu_reserve")


def get_cu_reserve() -> int:
    return int(load().uz_get_cu_reserve())


def mfma_clock_ghz(settle_s: float = 0.6, iters: int = 40000) -> dict:
    """uz_clock_probe(): shader clock held under a dense bf16 MFMA stream on every CU, after `settle_s` seconds of that
    same load (the DVFS controller needs time); median / min / max over the 256 workgroups of the last launch, and the
    bf16 TFLOP/s the probe itself sustained.  Runs ~1 s; bench.py calls it OUTSIDE the timed region."""
    import time
    lib = load()
    dev = torch.device("cuda", torch.cuda.current_device())
    out = torch.zeros(256, 2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    t_end = time.perf_counter() + settle_s
    while time.perf_counter() < t_end:
        for _ in range(4):
            check(lib.uz_clock_probe(iters, out.data_ptr(), 256, stream_ptr()), "uz_clock_probe")
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib.uz_clock_probe(iters, out.data_ptr(), 256, stream_ptr()), "uz_clock_probe")
    e1.record()
    torch.cuda.synchronize()
    o = out.double().cpu()
    ghz = (o[:, 0] / o[:, 1] / 10.0)
    flops = 256.0 * 8 * iters * 8 * 2.0 * 16 * 16 * 32
    return {"median_ghz": round(float(ghz.median()), 4), "min_ghz": round(float(ghz.min()), 4),
            "max_ghz": round(float(ghz.max()), 4),
            "probe_tflops": round(flops / (e0.elapsed_time(e1) * 1e-3) / 1e12, 1)}


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return UZ_F32
    if dt == torch.bfloat16:
        return UZ_BF16
    raise ValueError(f"unsupported run dtype {dt}; use torch.float32 or torch.bfloat16")


def require_cuda(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HipLibraryError(
                "unet_zoo_amd kernels run on an MI355X only: got a CPU tensor. Move the model and "
                "inputs to 'cuda' (there is no CPU fallback in the product path).")
