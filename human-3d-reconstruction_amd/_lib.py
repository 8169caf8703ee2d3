"""ctypes binding of csrc/libh3d_hip.so (C ABI: include/h3d.h).

There is deliberately NO fallback: if the HIP library is missing or an entry point is absent,
importing/using the compute path raises.  PyTorch is used by callers only for device memory,
streams and torch.distributed.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libh3d_hip.so")

H3D_F32, H3D_BF16, H3D_F16, H3D_F16X3 = 0, 1, 2, 3
OP_STEM, OP_CONV, OP_DCN, OP_MAXPOOL, OP_UPADD, OP_COPY, OP_HEADS, OP_DCN_V1, OP_DCN_FUSED = 1, 2, 3, 4, 5, 6, 7, 8, 9
OP_CONV_STREAM, OP_DCN_FUSED_F16, OP_DCN_FUSED_STREAM, OP_STEM3, OP_UPDCN_F16 = 10, 11, 12, 13, 14
OP_IM2COL, OP_MAXPOOL3, OP_DEPTH2SPACE = 15, 16, 17
HEADS_MAX = 16
OUT_NHWC, OUT_NCHW_F32, OUT_NHWC_F32, OUT_NHWC_F16 = 0, 1, 2, 3
DCN_INPUT_NHWC, DCN_OUTPUT_NHWC, DCN_F32_MFMA = 1, 2, 4
ABI_VERSION = 4

# h3d_op.reserved: the flag catalogue of include/h3d.h under the same names minus the H3D_ prefix (what each flag requires of the
# buffers is stated there).  OPF_* = operand / plan flags, TUNE_* = tuning overrides of tests and tools.
DCN_AUX_BYTES = 256
DCN_FUSED_BIAS_WMAX, DCN_FUSED_BIAS_AMAX = 32, 34       # float offsets behind `rows` in h3d_dcn_fused_pack_f32_cached's bias_out
OPF_DCN_MASK_FINAL, OPF_DCN_RAW_PACK, OPF_DCN_ACT_MAXIMA, TUNE_DCN_ABLATE_MASK = 0x800, 0x100000, 0x200000, 0x1f
OPF_DCN_FUSED_RAW_PACK, OPF_DCN_FUSED_SCALED_INPUT = 0x100000, 0x200000
TUNE_DCN_FUSED_X3_MARGIN2, TUNE_DCN_FUSED_X3_MARGIN6, TUNE_DCN_FUSED_X3_MARGIN4, TUNE_DCN_FUSED_X3_ABLATE_MASK = 0x2000, 0x4000, 0x8000, 0x1f
OPF_DCN_STREAM_NO_SLOTS, OPF_DCN_STREAM_WIDE_MARGIN, OPF_DCN_STREAM_SLOTS512, OPF_DCN_STREAM_F16_INPUT = 0x1000, 0x8000, 0x10000, 0x40000
OPF_DCN_STREAM_STATS, OPF_DCN_STREAM_VARIANT_MASK = 0x20000, 0x58600
TUNE_DCN_STREAM_FORCE_NARROW_WG, TUNE_DCN_STREAM_FORCE_WIDE_WG = 0x200, 0x400
TUNE_DCN_STREAM_F16_DCN5, TUNE_DCN_STREAM_F16_KEEP_DCN3, TUNE_DCN_STREAM_ABLATE_MASK = 0x4000, 0x2000, 0x1f
TUNE_DCN_STREAM_X3_MARGIN2, TUNE_DCN_STREAM_X3_MARGIN3, TUNE_DCN_STREAM_X3_MARGIN4, TUNE_DCN_STREAM_X3_ABLATE_MASK = 0x4000, 0x8000, 0x10000, 0x1f
TUNE_DCN_F16_ONE_WG_PER_CU, TUNE_DCN_F16_ABLATE_MASK = 0x100, 0xff
TUNE_CONV_STREAM_TILE_MASK, TUNE_CONV_STREAM_AUTO, TUNE_CONV_STREAM_ROUND4_RULE, TUNE_CONV_STREAM_ABLATE_MASK = 0xffff, 1, 0x10000000, 0x1f0000
TUNE_CONV_TILE, TUNE_CONV_HALO_TILE, TUNE_CONV_FORCE_GEMM, TUNE_CONV_GEMM_TILE_MASK = 0x1000, 0x2000, 0x4000, 0xf00
TUNE_CONV_X3_TILED, TUNE_CONV_X3_TILE_MASK, TUNE_CONV_X3_CK16, TUNE_CONV_X3_MT2 = 0x1000, 0x1fff, 0x2000, 0x4000
TUNE_UPADD_TAPS_GLOBAL, TUNE_UPADD_TAPS_LDS, OPF_UPADD_FOLDED = 1, 2, 0x100
OPF_TREE_ENTRY, OPF_TREE_ENTRY_PRIVATE_POOL = 0x20000000, 0x40000000
TUNE_HEADS_SEPARATE_BIAS, TUNE_HEADS_ABLATE_MASK = 0x200, 0xff
TUNE_HEADS_SPARSE_LDS_PATCH, TUNE_HEADS_SPARSE_WAVES4 = 0x400, 0x800


def TUNE_DCN_STREAM_DCN5_XP(xp):
    return xp << 16


def TUNE_DCN_STREAM_DCN5_XP_OF(reserved):
    return (reserved >> 16) & 0xff


def TUNE_CONV_STREAM_TILE(variant, mt, waves):
    return variant << 12 | mt << 8 | waves


def TUNE_CONV_STREAM_ABLATE(bits):
    return bits << 16


def TUNE_CONV_STREAM_ABLATE_OF(reserved):
    return (reserved & TUNE_CONV_STREAM_ABLATE_MASK) >> 16


def TUNE_CONV_1X1_TILE(mt, th):
    return TUNE_CONV_TILE | mt << 4 | th >> 3


def TUNE_CONV_1X1_TILE_MT(reserved):
    return (reserved >> 4) & 15


def TUNE_CONV_1X1_TILE_TH(reserved):
    return (reserved & 15) * 8


def TUNE_CONV_GEMM_TILE(n):
    return n << 8


def TUNE_CONV_X3_TILE(mt, waves, th):
    return TUNE_CONV_X3_TILED | mt << 8 | waves << 4 | th >> 3

c_vp, c_i, c_fp = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p


class H3dOp(ctypes.Structure):
    """Mirror of `struct h3d_op` in include/h3d.h."""
    _fields_ = [
        ("kind", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("in_", c_vp), ("in2", c_vp), ("w", c_vp), ("bias", c_vp), ("out", c_vp),
        ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
        ("Cin", ctypes.c_int32), ("in_cs", ctypes.c_int32), ("in2_cs", ctypes.c_int32),
        ("Ho", ctypes.c_int32), ("Wo", ctypes.c_int32),
        ("Cout", ctypes.c_int32), ("out_cs", ctypes.c_int32),
        ("ksize", ctypes.c_int32), ("stride", ctypes.c_int32), ("relu", ctypes.c_int32),
        ("out_mode", ctypes.c_int32), ("wrows", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("wexp", ctypes.c_int32), ("wexp2", ctypes.c_int32),
    ]


class _HeadEntry(ctypes.Structure):
    _fields_ = [("w2", c_vp), ("b2", c_vp), ("out", c_vp), ("C", ctypes.c_int32), ("wexp2", ctypes.c_int32)]


class H3dHeadsDesc(ctypes.Structure):
    """Mirror of `struct h3d_heads_desc` (host-side descriptor behind H3D_OP_HEADS)."""
    _fields_ = [("nheads", ctypes.c_int32), ("wexp", ctypes.c_int32), ("head", _HeadEntry * HEADS_MAX)]


HEADS_LISTS_MAX = 4


class H3dHeadsList(ctypes.Structure):
    """Mirror of `struct h3d_heads_list` (one position list of h3d_heads_sparse_lists)."""
    _fields_ = [("inds", c_vp), ("K", ctypes.c_int32), ("head_mask", ctypes.c_uint32)]


class H3dUpdcnDesc(ctypes.Structure):
    """Mirror of `struct h3d_updcn_desc` (host-side descriptor behind H3D_OP_UPDCN_F16)."""
    _fields_ = [("skip", c_vp), ("w_up", c_vp), ("w_off", c_vp), ("skip_cs", ctypes.c_int32), ("reserved", ctypes.c_int32)]


TRAIN_BRIGHTNESS, TRAIN_CONTRAST, TRAIN_SATURATION = 0, 1, 2
TRAIN_INPUT_NO_COLOR_AUG = 1


class H3dTrainImage(ctypes.Structure):
    """Mirror of `struct h3d_train_image` in include/h3d.h (section 3b): 136 bytes, no padding."""
    _fields_ = [("minv", ctypes.c_double * 6), ("light", ctypes.c_double * 3), ("offset", ctypes.c_int64),
                ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("row_bytes", ctypes.c_int32), ("flipped", ctypes.c_int32),
                ("order", ctypes.c_int32 * 3), ("alpha", ctypes.c_float * 3), ("one_minus_alpha", ctypes.c_float * 3),
                ("reserved", ctypes.c_int32)]


SMPL_KP_MAX_K, SMPL_KP_MAX_NV = 32, 16              # H3D_SMPL_KP_MAX_K / H3D_SMPL_KP_MAX_NV
RENDER_NEGATE_Z, RENDER_CULL_BACK = 1, 2           # H3D_RENDER_NEGATE_Z / H3D_RENDER_CULL_BACK
RENDER_MAX_V, RENDER_MAX_SIDE = 13120, 16384        # H3D_RENDER_MAX_V / H3D_RENDER_MAX_SIDE
COCO_BBOX, COCO_KEYPOINTS, COCO_ROUND2 = 0, 1, 1      # H3D_COCO_BBOX / H3D_COCO_KEYPOINTS / H3D_COCO_ROUND2
COCO_MAX_D, COCO_MAX_G, COCO_SCAN_CHUNK = 128, 1024, 1024       # H3D_COCO_MAX_D / H3D_COCO_MAX_G / H3D_COCO_SCAN_CHUNK
MESH_EVAL_MAX_SWEEPS = 30                                       # H3D_MESH_EVAL_MAX_SWEEPS
CONV_BWD_RELU, CONV_BWD_MFMA_CMAX = 1, 2048        # H3D_CONV_BWD_RELU / H3D_CONV_BWD_MFMA_CMAX
ADAM_CAPACITY, ADAM_CHUNK = 48, 2048        # H3D_ADAM_CAPACITY / H3D_ADAM_CHUNK: tensors per launch, elements per workgroup


class H3dAdamTensor(ctypes.Structure):
    """Mirror of `struct h3d_adam_tensor` in include/h3d.h (section 7): 72 bytes."""
    _fields_ = [("param", c_vp), ("grad", c_vp), ("exp_avg", c_vp), ("exp_avg_sq", c_vp), ("n", ctypes.c_int64),
                ("one_minus_b1", ctypes.c_float), ("b2", ctypes.c_float), ("one_minus_b2", ctypes.c_float), ("bc2_sqrt", ctypes.c_float),
                ("eps", ctypes.c_float), ("neg_step_size", ctypes.c_float), ("weight_decay", ctypes.c_float)]


# name -> argtypes (restype is int unless noted); also the export list the CPU test checks
SIGNATURES = {
    "h3d_dcn_v2_forward": [c_vp] * 6 + [c_i] * 14 + [c_vp],
    "h3d_dcn_v2_forward_ws": [c_vp] * 6 + [c_i] * 14 + [c_vp, ctypes.c_size_t, c_vp],
    "h3d_dcn_v2_pack_weights": [c_vp, c_vp, c_i, c_i, c_i, c_vp, c_vp],
    "h3d_dcn_v2_pack_weights_cached": [c_vp, c_vp, c_i, c_i, c_i, c_vp, c_vp, c_vp],
    "h3d_dcn_fused_pack_f32_cached": [c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_vp, c_vp, c_vp, c_vp, c_vp],
    "h3d_dcn_v2_forward_packed": [c_vp] * 5 + [c_i] * 7 + [c_vp, ctypes.c_size_t, c_vp],
    "h3d_dcn_nchw_to_nhwc_scaled": [c_vp, c_vp] + [c_i] * 4 + [c_vp, c_vp],
    "h3d_dcn_v2_backward_workspace_bytes": [c_i] * 14 + [ctypes.POINTER(ctypes.c_size_t)],
    "h3d_dcn_v2_backward": [c_vp] * 11 + [c_i] * 14 + [c_vp, ctypes.c_size_t, c_vp],
    "h3d_dcn_v2_backward_general": [c_vp] * 11 + [c_i] * 14 + [c_vp, ctypes.c_size_t, c_vp],
    "h3d_dcn_offset_mask": [c_vp] * 5 + [c_i] * 11 + [c_vp],
    "h3d_dcn_v2_psroi_pooling_forward": [c_vp] * 5 + [c_i] * 7 + [ctypes.c_float] + [c_i] * 5 + [ctypes.c_float, c_vp],
    "h3d_dcn_pooling_modulated": [c_vp] * 4 + [c_i] * 5 + [ctypes.c_float] + [c_i] * 5 + [ctypes.c_float, c_vp],
    "h3d_dcn_v2_psroi_pooling_backward": [c_vp] * 7 + [c_i] * 8 + [ctypes.c_float] + [c_i] * 5 + [ctypes.c_float, c_i, c_vp],
    "h3d_dcn_pooling_modulated_backward": [c_vp] * 6 + [c_i] * 5 + [ctypes.c_float] + [c_i] * 5 + [ctypes.c_float, c_i, c_vp],
    "h3d_psroi_backward_path": [c_vp, c_vp] + [c_i] * 6 + [ctypes.c_float] + [c_i] * 3 + [ctypes.c_float, c_i, c_i, ctypes.POINTER(c_i)],
    "h3d_build_flags": [],
    "h3d_dcn_fused_ck": [c_i, c_i],
    "h3d_dcn_far_samples": [ctypes.POINTER(H3dOp), c_vp, c_vp],
    "h3d_smpl_pose_heads": [c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i, c_vp],
    "h3d_smpl_coef_pack": [c_vp, c_vp, c_i, c_i, c_vp, c_vp],
    "h3d_smpl_verts3": [c_vp] * 6 + [c_i] * 5 + [c_vp, c_vp],
    "h3d_smpl_verts3_exact": [c_vp] * 6 + [c_i] * 5 + [c_vp, c_vp],
    "h3d_preprocess": [c_vp, c_i, c_i, c_i, c_i, c_vp, c_vp, c_vp, c_i, c_i, c_vp, c_vp],
    # training input (include/h3d.h section 3b; h3d_amd/train_input.py)
    "h3d_train_input_workspace_bytes": [c_i] * 4 + [ctypes.POINTER(ctypes.c_size_t)],
    "h3d_train_input": [c_vp, ctypes.c_size_t, c_vp, c_vp, c_i, c_vp, c_vp, c_i, c_i, c_i, c_vp, ctypes.c_size_t, c_vp, c_vp, c_vp],
    "h3d_run_ops": [ctypes.POINTER(H3dOp), c_i, c_vp],
    "h3d_run_ops_timed": [ctypes.POINTER(H3dOp), c_i, c_vp, c_vp],
    "h3d_op_kernel_name": [ctypes.POINTER(H3dOp), ctypes.c_char_p, c_i],
    "h3d_heads_sparse": [ctypes.POINTER(H3dOp), c_vp, c_i, c_vp],
    "h3d_heads_sparse_lists": [ctypes.POINTER(H3dOp), c_i, ctypes.POINTER(H3dHeadsList), c_vp],
    "h3d_nchw_f32_to_nhwc": [c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_i, c_vp],
    "h3d_nhwc_to_nchw_f32": [c_vp, c_i, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp],
    "h3d_nms_topk": [c_vp, c_i, c_i, c_i, c_i, c_i, c_i, c_vp, c_vp, c_vp, c_vp, c_vp],
    "h3d_nms_topk2": [c_vp, c_i, c_vp, c_vp, c_vp, c_vp, c_vp, c_i, c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp],
    "h3d_nms_topk_large": [c_vp, c_i, c_i, c_i, c_i, c_i, c_i, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_size_t, c_vp],
    "h3d_nms": [c_vp, c_i, c_i, c_i, c_i, c_vp, c_vp],
    "h3d_topk_merge": [c_vp] * 4 + [c_i] * 3 + [c_vp] * 5 + [c_vp],
    "h3d_gather_feat": [c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp, c_vp],
    "h3d_multi_pose_assemble": [c_vp] * 13 + [c_i] * 5 + [c_vp, c_vp],
    "h3d_ctdet_assemble": [c_vp] * 7 + [c_i] * 6 + [c_vp, c_vp],
    "h3d_multi_pose_post_process": [c_vp] * 3 + [c_i] * 5 + [c_vp, c_vp],
    "h3d_smpl_pose": [c_vp] * 5 + [c_i] + [c_vp] * 4 + [c_i, c_vp],
    "h3d_smpl_verts": [c_vp] * 8 + [c_i] * 4 + [c_vp, c_vp],
    "h3d_smpl_verts2": [c_vp] * 7 + [c_i] * 5 + [c_vp, c_vp],
    "h3d_sigmoid_clamp": [c_vp, c_vp, ctypes.c_size_t, c_vp],
    # losses (h3d_amd/losses.py holds the mirror of `struct h3d_loss_term`)
    "h3d_loss_workspace_bytes": [c_vp, c_i, ctypes.POINTER(ctypes.c_size_t)],
    "h3d_loss_forward": [c_vp, c_i, c_vp, c_vp, ctypes.c_size_t, c_vp],
    "h3d_loss_backward": [c_vp, c_i, c_vp, c_vp, c_vp],
    # SMPL backward (include/h3d.h section 4b)
    "h3d_smpl_backward_workspace_bytes": [c_i] * 5 + [ctypes.POINTER(ctypes.c_size_t)],
    "h3d_smpl_backward": [c_vp] * 12 + [c_i] * 4 + [c_vp, c_vp, c_vp, ctypes.c_size_t, c_vp],
    "h3d_smpl_heads_backward": [c_vp] * 3 + [c_i] * 4 + [c_vp] * 10 + [c_i] * 3 + [c_vp, c_vp, c_vp, ctypes.c_size_t, c_vp],
    # SMPL keypoint reprojection loss (include/h3d.h section 4c; h3d_amd/smpl_loss.py)
    "h3d_smpl_kp_loss_workspace_bytes": [c_i, c_i, ctypes.POINTER(ctypes.c_size_t)],
    "h3d_smpl_kp_loss_forward": [c_vp] * 6 + [c_i] + [c_vp] * 3 + [c_i] * 7 + [c_vp] * 4 + [ctypes.c_size_t, c_vp],
    "h3d_smpl_kp_loss_backward": [c_vp] * 6 + [c_i] + [c_vp] * 7 + [c_i] * 7 + [c_vp] * 4,
    # SMPL 3D supervision (include/h3d.h section 4e; h3d_amd/smpl_sup.py)
    "h3d_smpl_sup_labels": [c_vp] * 10 + [c_i] * 3 + [c_vp] * 7,
    "h3d_smpl_sup_loss_workspace_bytes": [c_i, c_i, ctypes.POINTER(ctypes.c_size_t)],
    "h3d_smpl_sup_loss_forward": [c_vp] * 10 + [c_i] * 4 + [c_vp, c_vp, ctypes.c_size_t, c_vp],
    "h3d_smpl_sup_loss_backward": [c_vp] * 10 + [c_i] * 4 + [c_vp] * 6,
    # mesh rendering (include/h3d.h section 4d; h3d_amd/render.py)
    "h3d_render_workspace_bytes": [c_i] * 3 + [ctypes.POINTER(ctypes.c_size_t)],
    "h3d_render_rasterize": [c_vp] * 6 + [c_i] * 9 + [c_vp, c_vp, c_vp, ctypes.c_size_t, c_vp],
    "h3d_render_shade": [c_vp] * 5 + [c_i] * 6 + [ctypes.c_float, ctypes.c_float, c_i, c_i, c_vp, c_vp],
    # heads backward (include/h3d.h section 2b; h3d_amd/heads.py holds the mirror of `struct h3d_heads_bwd_head`)
    "h3d_heads_backward_workspace_bytes": [c_i] * 5 + [c_vp, ctypes.POINTER(ctypes.c_size_t)],
    "h3d_heads_backward": [c_vp] + [c_i] * 6 + [c_vp, c_vp, c_vp, ctypes.c_size_t, c_vp],
    # convolution backward (include/h3d.h section 2c; h3d_amd/conv.py)
    "h3d_conv2d_backward_workspace_bytes": [c_i] * 14 + [ctypes.POINTER(ctypes.c_size_t)],
    "h3d_conv2d_backward": [c_vp, c_i, c_vp, c_vp, c_i, c_vp, c_i] + [c_vp] * 4 + [c_i] * 14 + [c_vp, ctypes.c_size_t, c_vp],
    "h3d_conv2d_backward_general": [c_vp, c_i, c_vp, c_vp, c_i, c_vp, c_i] + [c_vp] * 4 + [c_i] * 14 + [c_vp, ctypes.c_size_t, c_vp],
    # max-pool and up-sample + add backward (include/h3d.h section 2d; h3d_amd/pool_up.py)
    "h3d_maxpool2_backward": [c_vp, c_i, c_vp, c_i, c_vp, c_i] + [c_i] * 4 + [c_vp],
    "h3d_upsample_backward_workspace_bytes": [c_i] * 5 + [ctypes.POINTER(ctypes.c_size_t)],
    "h3d_upsample_backward": [c_vp, c_i, c_vp, c_vp, c_i, c_vp, c_i, c_vp] + [c_i] * 5 + [c_vp, ctypes.c_size_t, c_vp],
    # BatchNorm with batch statistics (include/h3d.h section 2e; h3d_amd/bn.py)
    "h3d_batch_norm_workspace_bytes": [c_i] * 4 + [ctypes.POINTER(ctypes.c_size_t)],
    "h3d_batch_norm_plan": [c_i] * 4 + [ctypes.POINTER(c_i), ctypes.POINTER(c_i)],
    "h3d_batch_norm_forward": [c_vp, c_i, c_vp, c_vp, c_vp, c_i, c_vp, c_i] + [c_vp] * 5 + [c_i] * 6 + [ctypes.c_float, ctypes.c_float, c_vp,
                               ctypes.c_size_t, c_vp],
    "h3d_batch_norm_backward": [c_vp, c_i, c_vp, c_i, c_vp, c_i, c_vp, c_vp, c_vp, c_vp, c_i, c_vp, c_i, c_vp, c_vp] + [c_i] * 6 +
                               [c_vp, ctypes.c_size_t, c_vp],
    # training targets (include/h3d.h section 6; h3d_amd/targets.py)
    "h3d_targets_workspace_bytes": [c_i] * 3 + [ctypes.POINTER(ctypes.c_size_t)],
    "h3d_multi_pose_targets": [c_vp] * 8 + [c_i] * 7 + [c_vp] * 13 + [c_i, c_vp, ctypes.c_size_t, c_vp],
    "h3d_ctdet_targets": [c_vp] * 6 + [c_i] * 6 + [c_vp] * 9 + [c_i, c_vp, ctypes.c_size_t, c_vp],
    # optimiser (include/h3d.h section 7; h3d_amd/optim.py)
    "h3d_adam_step": [ctypes.POINTER(H3dAdamTensor), c_i, c_vp],
    # evaluation (include/h3d.h section 8; h3d_amd/coco_eval.py)
    "h3d_coco_match_workspace_bytes": [c_i] * 3 + [ctypes.POINTER(ctypes.c_size_t)],
    "h3d_coco_match": [c_vp, c_i] + [c_vp] * 8 + [c_i] * 6 + [c_vp, c_i, c_vp, c_i] + [c_vp] * 11 + [ctypes.c_size_t, c_vp],
    "h3d_coco_accumulate_workspace_bytes": [c_i, c_i, ctypes.POINTER(ctypes.c_size_t)],
    "h3d_coco_accumulate": [c_vp] * 8 + [c_i] * 6 + [ctypes.POINTER(ctypes.c_int32), c_i, c_vp, c_i, c_vp, c_vp, c_vp, ctypes.c_size_t, c_vp],
    # 3D evaluation (include/h3d.h section 8b; h3d_amd/mesh_eval.py)
    "h3d_pointset_errors": [c_vp, c_i, c_vp, c_i, c_i, c_vp, c_vp, c_i, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_vp, c_vp, c_vp, c_vp],
    "h3d_metric_means": [c_vp, c_vp, c_i, c_vp, c_vp, c_vp],
}

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raise loudly when the library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "h3d_amd: HIP library not built (%s). Run `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C human-3d-reconstruction_amd/csrc`. There is no CPU fallback."
                % LIB_PATH)
        # PyTorch first: its wheel bundles its own HIP / HSA runtime, and libh3d_hip.so must bind to THAT copy (same
        # SONAME once it is loaded).  Loaded the other way round, the process ends up with two runtimes and the first
        # launch fails with "no ROCm-capable device is detected" (seen with build() followed by smoke() in one process).
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        L.h3d_last_error.restype = ctypes.c_char_p
        L.h3d_last_error.argtypes = []
        L.h3d_abi_version.restype = c_i
        if L.h3d_abi_version() != ABI_VERSION:
            raise RuntimeError("h3d_amd: libh3d_hip.so ABI %d != binding ABI %d"
                               % (L.h3d_abi_version(), ABI_VERSION))
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the export is missing
            fn.argtypes = args
            fn.restype = c_i
        L.h3d_dcn_v2_workspace_bytes.argtypes = [c_i] * 5
        L.h3d_dcn_v2_workspace_bytes.restype = ctypes.c_size_t
        L.h3d_dcn_v2_packed_weight_bytes.argtypes = [c_i] * 3
        L.h3d_dcn_v2_packed_weight_bytes.restype = ctypes.c_size_t
        L.h3d_dcn_v2_packed_workspace_bytes.argtypes = [c_i] * 5
        L.h3d_dcn_v2_packed_workspace_bytes.restype = ctypes.c_size_t
        L.h3d_nms_topk_large_workspace_bytes.argtypes = [c_i] * 5
        L.h3d_nms_topk_large_workspace_bytes.restype = ctypes.c_size_t
        _lib = L
    return _lib


def has_extra():
    """True when libh3d_hip.so was built with `make EXTRA=1` (the superseded kernel generations are in: csrc/Makefile)."""
    return bool(lib().h3d_build_flags() & 1)


_ERR_NAMES = {-1: "shape", -2: "dtype", -3: "launch", -4: "unsupported", -5: "argument"}


def check(rc, what):
    if rc != 0:
        msg = lib().h3d_last_error().decode("utf-8", "replace")
        raise RuntimeError("%s failed (%s error): %s" % (what, _ERR_NAMES.get(rc, rc), msg))


def workspace(size_fn, *args, device, min_bytes=0, what=None):
    """A uint8 workspace on `device` of what `size_fn(*args, &bytes)` asks for, at least `min_bytes`; None when that is nothing.
    `what` names the call in an error (default: the function's name)."""
    import torch
    n = ctypes.c_size_t(0)
    check(size_fn(*args, ctypes.byref(n)), what or size_fn.__name__)
    nbytes = max(n.value, min_bytes)
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def stream_ptr():
    """Raw hipStream_t of torch's current stream (the reference launches on the current
    stream too, dcn_v2_cuda.cu:108)."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            # the reference raises "Not implemented on the CPU" (DCNv2/src/dcn_v2.h:38)
            raise RuntimeError("Not implemented on the CPU")
