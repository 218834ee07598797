"""ctypes binding of ``libmi355yolo.so`` (C-ABI declared in ``include/mi355yolo.h``).

There is deliberately NO fallback: if the shared library is missing or a symbol cannot be resolved the
import of this module raises, and ``m355_create`` fails on a machine without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmi355yolo.so")


class M355Error(RuntimeError):
    """Raised when a libmi355yolo call returns a negative status."""


class ModelDesc(C.Structure):
    _fields_ = [("scale", C.c_int), ("nc", C.c_int), ("in_h", C.c_int), ("in_w", C.c_int),
                ("max_batch", C.c_int)]


class ConvInfo(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("cin", C.c_int), ("cout", C.c_int), ("k", C.c_int),
                ("stride", C.c_int), ("has_bn", C.c_int), ("transposed", C.c_int), ("act", C.c_int),
                ("groups", C.c_int)]


class OpInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 48), ("layer", C.c_char * 64), ("flops_per_image", C.c_double),
                ("bytes_per_image", C.c_double), ("weight_bytes", C.c_double)]


class AugParams(C.Structure):
    """m355_aug_params (include/mi355yolo.h)."""
    _fields_ = [("src", C.c_int32 * 4), ("xc", C.c_float), ("yc", C.c_float), ("minv", C.c_float * 6),
                ("hgain", C.c_float), ("sgain", C.c_float), ("vgain", C.c_float), ("flip", C.c_int32), ("mosaic", C.c_int32)]


class AugLayer(C.Structure):
    """m355_aug_layer (include/mi355yolo.h)."""
    _fields_ = [("src", C.c_int32 * 4), ("xc", C.c_float), ("yc", C.c_float), ("minv", C.c_float * 9), ("mosaic", C.c_int32),
                ("poly_first", C.c_int32), ("poly_count", C.c_int32)]


class AugExParams(C.Structure):
    """m355_aug_ex_params (include/mi355yolo.h)."""
    _fields_ = [("layer", AugLayer * 2), ("n_layers", C.c_int32), ("mix", C.c_float), ("hgain", C.c_float), ("sgain", C.c_float),
                ("vgain", C.c_float), ("flip", C.c_int32), ("flipud", C.c_int32)]


class AugPoly(C.Structure):
    """m355_aug_poly (include/mi355yolo.h)."""
    _fields_ = [("vert_first", C.c_int32), ("vert_count", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32),
                ("y1", C.c_int32)]


AUG_MAX_PASTE = 32            # M355_AUG_MAX_PASTE
AUG_MAX_POLY_VERTS = 1024     # M355_AUG_MAX_POLY_VERTS


class ConvLaunchArgs(C.Structure):
    """m355_conv_args (include/mi355yolo.h)."""
    _fields_ = [("x", C.c_void_p), ("x_bstride", C.c_int64), ("ldx", C.c_int32), ("hi", C.c_int32), ("wi", C.c_int32),
                ("cin", C.c_int32), ("w_packed", C.c_void_p), ("kpad", C.c_int32), ("bias", C.c_void_p),
                ("y", C.c_void_p), ("y_bstride", C.c_int64), ("ldy", C.c_int32), ("ho", C.c_int32), ("wo", C.c_int32),
                ("cout", C.c_int32), ("res", C.c_void_p), ("r_bstride", C.c_int64), ("ldr", C.c_int32),
                ("ksize", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("batch", C.c_int32),
                ("act", C.c_int32), ("out_f32", C.c_int32), ("convt_co", C.c_int32), ("tmode", C.c_int32),
                ("zero_page", C.c_void_p)]


class WgradLaunchArgs(C.Structure):
    """m355_wgrad_args (include/mi355yolo.h)."""
    _fields_ = [("dz", C.c_void_p), ("dz_bstride", C.c_int64), ("lddz", C.c_int32), ("x", C.c_void_p),
                ("x_bstride", C.c_int64), ("ldx", C.c_int32), ("hi", C.c_int32), ("wi", C.c_int32), ("cin", C.c_int32),
                ("ho", C.c_int32), ("wo", C.c_int32), ("cout", C.c_int32), ("ksize", C.c_int32), ("stride", C.c_int32),
                ("pad", C.c_int32), ("batch", C.c_int32), ("dw", C.c_void_p), ("zero_page", C.c_void_p), ("ws", C.c_void_p),
                ("ws_bytes", C.c_int64)]


class LetterboxImage(C.Structure):
    """m355_letterbox_image (include/mi355yolo.h)."""
    _fields_ = [("offset", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("uh", C.c_int32), ("uw", C.c_int32),
                ("top", C.c_int32), ("left", C.c_int32)]


class DfinePreImage(C.Structure):
    """m355_dfine_pre_image (include/mi355yolo.h)."""
    _fields_ = [("offset", C.c_int64), ("in_h", C.c_int32), ("in_w", C.c_int32), ("htab", C.c_int32), ("vtab", C.c_int32),
                ("mid_row", C.c_int32), ("reserved", C.c_int32)]


class DfinePreAxis(C.Structure):
    """m355_dfine_pre_axis (include/mi355yolo.h)."""
    _fields_ = [("in_size", C.c_int32), ("out_size", C.c_int32), ("ksize", C.c_int32), ("offset", C.c_int32)]


class DfineOptimRow(C.Structure):
    """m355_dfine_optim_row (include/mi355yolo.h)."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("numel", C.c_int64),
                ("chunk0", C.c_int32), ("lr", C.c_float), ("weight_decay", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("step_size", C.c_float), ("bc2_sqrt", C.c_float), ("one_minus_beta1", C.c_float),
                ("one_minus_beta2", C.c_float), ("decay", C.c_float), ("reserved", C.c_int32 * 3)]


DFINE_OPTIM_CHUNK = 4096          # M355_DFINE_OPTIM_CHUNK
DFINE_OPTIM_MAX_TENSORS = 65536   # M355_DFINE_OPTIM_MAX_TENSORS
DFINE_OPTIM_ADAM, DFINE_OPTIM_ADAMW = 0, 1
DFINE_PRE_MAX_TAPS = 64       # M355_DFINE_PRE_MAX_TAPS
DFINE_PRE_MAX_W = 4096        # M355_DFINE_PRE_MAX_W
DFINE_PRE_MAX_H = 16384       # M355_DFINE_PRE_MAX_H


# symbol -> (restype, argtypes); every entry of include/mi355yolo.h
_P = C.c_void_p
_F = C.POINTER(C.c_float)
SIGNATURES = {
    "m355_version": (C.c_char_p, []),
    "m355_last_error": (C.c_char_p, [_P]),
    "m355_create": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(_P)]),
    "m355_destroy": (None, [_P]),
    "m355_num_convs": (C.c_int, [_P]),
    "m355_get_conv_info": (C.c_int, [_P, C.c_int, C.POINTER(ConvInfo)]),
    "m355_num_anchors": (C.c_int, [_P]),
    "m355_pred_width": (C.c_int, [_P]),
    "m355_proto_hw": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "m355_workspace_bytes": (C.c_size_t, [_P]),
    "m355_flops_per_image": (C.c_double, [_P]),
    "m355_set_conv_weights": (C.c_int, [_P, C.c_int, _P, _P]),
    "m355_forward": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "m355_num_ops": (C.c_int, [_P]),
    "m355_get_op_info": (C.c_int, [_P, C.c_int, C.POINTER(OpInfo)]),
    "m355_set_profiling": (C.c_int, [_P, C.c_int]),
    "m355_collect_op_times": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_long)]),
    "m355_get_raw_head": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int)]),
    "m355_copy_raw_head": (C.c_int, [_P, C.c_int, _P, _P]),
    "m355_set_keep_raw": (C.c_int, [_P, C.c_int]),
    "m355_postprocess": (C.c_int, [_P, _P, _P, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P, _P, _P]),
    "m355_conv2d_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int,
                                  C.c_int, _P, _P, C.c_int, C.c_int, _P]),
    "m355_c2f_c32_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P]),
    "m355_bneck_pair_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P, C.c_int, _P]),
    "m355_conv3x3_blockdiag_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "m355_planes_diag_pack": (C.c_long, [C.c_int, _P, _P, _P, _P, C.c_long]),
    "m355_s2c64_cv1_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    "m355_stem_s2c32_cv1_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P]),
    "m355_proto_phase_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "m355_head_tail_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "m355_tal_assign_launch": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "m355_conv2d_dgrad": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "m355_conv2d_wgrad": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "m355_bn_silu_train_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_float, C.c_int, _P, _P, _P, _P, _P]),
    "m355_bn_silu_train_bwd": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P]),
    "m355_bn_workspace_floats": (C.c_size_t, [C.c_int]),
    "m355_wgrad_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "m355_grad_sumsq_workspace_floats": (C.c_size_t, []),
    "m355_convt2x2_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P]),
    "m355_stem_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P]),
    "m355_stem6_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P]),
    "m355_dwconv3x3_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_int, _P]),
    "m355_psa_attn_fwd": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "m355_sppf_pool": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "m355_upsample2x": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "m355_head_decode": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "m355_head_decode_ex": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "m355_nms": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P, _P]),
    "m355_conv_launch": (C.c_int, [C.POINTER(ConvLaunchArgs), _P]),
    "m355_wgrad_launch": (C.c_int, [C.POINTER(WgradLaunchArgs), _P]),
    "m355_bn_train_fwd_launch": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.c_float, C.c_int32, _P, C.c_int32,
                                           _P, C.c_int32, _P, _P, _P, _P, _P, C.c_float, _P]),
    "m355_bn_train_bwd_launch": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32,
                                           _P, C.c_int32, _P, _P, _P]),
    "m355_adamw_step": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                  C.c_float, C.c_int32, C.c_float, C.c_float, _P]),
    "m355_sgd_step": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_float,
                                C.c_float, C.c_float, _P]),
    "m355_grad_sumsq": (C.c_int, [_P, C.c_int64, _P, _P]),
    "m355_augment": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "m355_augment_ex_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "m355_augment_ex": (C.c_int, [_P, C.c_int32, C.POINTER(AugExParams), C.POINTER(AugPoly), C.c_int32, _F, C.c_int32, _P, C.c_int64,
                                  _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "m355_msda_forward": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, C.c_int32,
                                    C.c_int32, C.c_int32, _P, _P]),
    "m355_msda_module_forward": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, _P,
                                           C.c_int32, C.c_int32, C.c_float, _P, _P]),
    "m355_dfine_decode": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, C.c_int32, _P]),
    "m355_msda_backward_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "m355_msda_backward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, C.c_int32,
                                     C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64, _P]),
    "m355_msda_module_backward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, _P,
                                            C.c_int32, C.c_int32, C.c_float, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "m355_dfine_decode_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, C.c_int32, _P]),
    "m355_dfine_match_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "m355_dfine_match": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float,
                                   C.c_float, C.c_float, C.c_int32, _P, C.c_int64, _P, _P, _P, C.c_int32, _P, _P]),
    "m355_dfine_postprocess": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_float, _P, _P, _P, _P, _P]),
    "m355_dfine_preprocess": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int64, _P, C.c_int32, C.c_int32,
                                        _P, C.c_int64, _P, _P]),
    "m355_dfine_select_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "m355_dfine_select_forward": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64, _P, _P, _P,
                                            _P, _P, _P, _P]),
    "m355_dfine_select_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                             _P]),
    "m355_dfine_loss_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "m355_dfine_loss_forward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, C.c_int32,
                                          C.c_float, C.c_float, C.c_float, _P, _P, _P, _P, _P, C.c_int32, C.c_float, C.c_float,
                                          _P, C.c_int64, _P, _P]),
    "m355_dfine_loss_backward": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, C.c_int32,
                                           C.c_float, C.c_float, C.c_float, _P, _P, _P, _P, _P, C.c_int32, C.c_float, C.c_float,
                                           _P, _P, _P, _P, _P]),
    "m355_dfine_attn_forward": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_int32, _P, _P, _P]),
    "m355_dfine_attn_backward": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_int32,
                                           _P, _P]),
    "m355_dfine_addln_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "m355_dfine_addln_forward": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_uint64, C.c_int32, _P, _P, _P,
                                           _P]),
    "m355_dfine_addln_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, C.c_uint64, C.c_int32, _P, _P, _P,
                                            _P, _P, C.c_int64, _P]),
    "m355_dfine_relu_dropout_forward": (C.c_int, [_P, C.c_int64, C.c_float, C.c_uint64, C.c_int32, _P, _P]),
    "m355_dfine_relu_dropout_backward": (C.c_int, [_P, _P, C.c_int64, C.c_float, C.c_uint64, C.c_int32, _P, _P]),
    "m355_dfine_dropout_mask": (C.c_int, [C.c_int64, C.c_float, C.c_uint64, C.c_int32, _P, _P]),
    "m355_dfine_addln_clamp_forward": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_float, _P, _P, _P, _P]),
    "m355_dfine_addln_clamp_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, C.c_float, _P, _P, _P, _P,
                                                  _P, C.c_int64, _P]),
    "m355_dfine_gate_ln_forward": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, _P, _P, _P, _P]),
    "m355_dfine_gate_ln_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int64,
                                              _P]),
    "m355_dfine_lqe_forward": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P]),
    "m355_dfine_lqe_backward": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    "m355_dfine_query_pos_forward": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, _P, _P]),
    "m355_dfine_query_pos_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "m355_dfine_query_pos_backward": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, _P, _P, _P, _P, C.c_int64, _P]),
    "m355_dfine_refine_reference_forward": (C.c_int, [_P, _P, C.c_int64, C.c_float, _P, _P]),
    "m355_dfine_refine_reference_backward": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "m355_dfine_refine_boxes_forward": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, _P, _P, _P]),
    "m355_dfine_refine_boxes_backward": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, _P, _P, _P]),
    "m355_dfine_maps_to_tokens": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "m355_dfine_tokens_to_maps": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "m355_dfine_gelu_forward": (C.c_int, [_P, C.c_int64, _P, _P]),
    "m355_dfine_gelu_backward": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "m355_dfine_gru_workspace_bytes":(C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "m355_dfine_gru_forward": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, C.c_int64, C.c_int32,
                                         _P, _P]),
    "m355_dfine_gru_backward": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64,
                                          _P, _P]),
    "m355_dfine_decode_guarded": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, C.c_int32, _P]),
    "m355_dfine_decode_guarded_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_float, C.c_int32, _P]),
    "m355_dfine_temporal_fuse_forward": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "m355_dfine_temporal_fuse_backward": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "m355_dfine_guard_logits_forward": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_float, _P, _P]),
    "m355_dfine_guard_logits_backward": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_float, _P, _P, _P]),
    "m355_dfine_noobject_loss_forward": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "m355_dfine_noobject_loss_backward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "m355_dfine_consistency_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "m355_dfine_consistency_loss_forward": (C.c_int, [_P, C.c_int32, C.c_int64, _P, C.c_int64, _P, _P]),
    "m355_dfine_consistency_loss_backward": (C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P]),
    "m355_dfine_grad_sumsq_launch": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int64, _P]),
    "m355_dfine_clip_scale_launch": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int64, C.c_float, _P, _P]),
    "m355_dfine_adam_launch": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int64, C.c_float, _P, _P]),
    "m355_repack_launch": (C.c_int, [_P, _P, C.c_int32, _P]),
    "m355_sppf_pool_bwd_launch": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int32, _P, C.c_int64,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "m355_sppf_pool_launch": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, _P]),
    "m355_sppf_pool_form": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "m355_upsample2x_launch": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, _P]),
    "m355_adown_pool_launch": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "m355_colsum_workspace_floats": (C.c_int64, [C.c_int64, C.c_int32]),
    "m355_colsum_launch": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P]),
    "m355_upsample2x_bwd_launch": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, _P]),
    "m355_addsilu_fwd_launch": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "m355_addsilu_bwd_launch": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int64, C.c_int32, _P]),
    "m355_adown_fwd_launch": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int32, _P, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, _P]),
    "m355_adown_bwd_launch": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int32, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_int32, _P]),
    "m355_u8_to_f16x8_launch": (C.c_int, [_P, _P, C.c_int64, _P]),
    "m355_mask_loss_launch": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                         C.c_int32, _P, _P]),
    "m355_box_loss_launch": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P]),
    "m355_dfl_decode_launch": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "m355_cls_bce_workspace_floats": (C.c_size_t, []),
    "m355_cls_bce_launch": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.c_int32, _P, _P, _P, _P]),
    "m355_proto_masks": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "m355_postprocess_ex": (C.c_int, [_P, _P, _P, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "m355_nms_ex": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, _P, _P, _P, _P]),
    "m355_proto_masks_native": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "m355_letterbox_u8": (C.c_int, [_P, C.POINTER(LetterboxImage), C.c_int, C.c_int, C.c_int, _P, _P]),
}


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  This package has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(rc: int, engine=None) -> None:
    if rc < 0:
        msg = lib.m355_last_error(engine)
        raise M355Error(f"libmi355yolo error {rc}: {msg.decode() if msg else '?'}")


def version() -> str:
    return lib.m355_version().decode()
