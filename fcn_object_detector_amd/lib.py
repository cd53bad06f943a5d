"""ctypes binding of libfcnhip.so (include/fcnhip.h).

The shipped path has no CPU fallback: if the HIP library is missing or fails to
load, every entry point raises :class:`FcnLibraryError`.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# $FCN_LIB_PATH selects another BUILD of the same HIP library (the stamped diagnostic build of tools/conv_timeline.py);
# there is still no CPU path behind it.
LIB_PATH = os.environ.get("FCN_LIB_PATH") or os.path.join(_HERE, "libfcnhip.so")


class FcnLibraryError(RuntimeError):
    pass


class FcnError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("libfcnhip error %d: %s" % (code, msg))
        self.code = code


class ConvDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("y", C.c_void_p), ("y2", C.c_void_p),
        ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("x_cstride", C.c_int32),
        ("Cout", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32), ("pad", C.c_int32), ("stride", C.c_int32),
        ("OH", C.c_int32), ("OW", C.c_int32),
        ("y_cstride", C.c_int32), ("y_coffset", C.c_int32), ("y2_cstride", C.c_int32), ("y2_coffset", C.c_int32),
        ("flags", C.c_int32), ("in_shift", C.c_float),
    ]


class ConvTail(C.Structure):
    _fields_ = [("n", C.c_int32), ("finalize", C.c_int32), ("heads", ConvDesc * 4), ("scratch", C.c_void_p), ("arrive", C.c_void_p)]


class ConvGroup(C.Structure):
    _fields_ = [("d_probs", C.c_void_p), ("n", C.c_int32), ("cfg", C.c_int32), ("total_tiles", C.c_int32)]


class TConvDesc(C.Structure):
    """fcn_tconv_desc: transposed convolution (group-1 Deconvolution forward / data gradient of a strided Convolution)."""
    _fields_ = [
        ("a", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("b", C.c_void_p), ("y2", C.c_void_p),
        ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Ca", C.c_int32), ("a_cstride", C.c_int32),
        ("Cb", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32), ("pad", C.c_int32), ("stride", C.c_int32),
        ("OH", C.c_int32), ("OW", C.c_int32),
        ("b_cstride", C.c_int32), ("b_coffset", C.c_int32), ("y2_cstride", C.c_int32), ("y2_coffset", C.c_int32),
        ("flags", C.c_int32),
    ]


class TConvPlan(C.Structure):
    _fields_ = [("d_probs", C.c_void_p), ("n", C.c_int32), ("cfg", C.c_int32), ("grid_x", C.c_int32), ("grid_y", C.c_int32),
                ("total_tiles", C.c_int32)]


class RConvDesc(C.Structure):
    """fcn_rconv_desc: rectangular or dilated convolution, geometry per axis (forward, data gradient on the flipped bank, weight gradient)."""
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("y", C.c_void_p), ("y2", C.c_void_p),
        ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("x_cstride", C.c_int32),
        ("Cout", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32), ("pad_h", C.c_int32), ("pad_w", C.c_int32),
        ("stride_h", C.c_int32), ("stride_w", C.c_int32), ("OH", C.c_int32), ("OW", C.c_int32),
        ("y_cstride", C.c_int32), ("y_coffset", C.c_int32), ("y2_cstride", C.c_int32), ("y2_coffset", C.c_int32),
        ("flags", C.c_int32), ("dilation", C.c_int32),
    ]


class RConvPlan(C.Structure):
    _fields_ = [("d_probs", C.c_void_p), ("n", C.c_int32), ("cfg", C.c_int32), ("grid_x", C.c_int32), ("grid_y", C.c_int32),
                ("total_tiles", C.c_int32)]


class DwConvDesc(C.Structure):
    """fcn_dwconv_desc: depthwise convolution, geometry per axis (forward f32 / f16, data gradient, weight gradient)."""
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("y", C.c_void_p), ("y2", C.c_void_p),
        ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("x_cstride", C.c_int32),
        ("kh", C.c_int32), ("kw", C.c_int32), ("pad_h", C.c_int32), ("pad_w", C.c_int32),
        ("stride_h", C.c_int32), ("stride_w", C.c_int32), ("OH", C.c_int32), ("OW", C.c_int32),
        ("y_cstride", C.c_int32), ("y_coffset", C.c_int32), ("y2_cstride", C.c_int32), ("y2_coffset", C.c_int32),
        ("flags", C.c_int32), ("dilation", C.c_int32),
    ]


def dwconv_desc(x: int, w: Optional[int], bias: Optional[int], y: int, n: int, h: int, wd: int, c: int, x_cstride: int, kh: int, kw: int,
                ph: int, pw: int, sh: int, sw: int, dilation: int, y_cstride: int, y_coffset: int, flags: int = 0) -> DwConvDesc:
    """fcn_dwconv_desc of the forward problem n x c x h x wd under a kh x kw window (pads ph / pw, strides sh / sw, one dilation): x the
    address of channel 0 of the input view, y the address of the output BUFFER (the slice starts y_coffset channels in); OH / OW by
    Caffe's rule."""
    d = DwConvDesc()
    d.x, d.w, d.bias, d.y = x, w, bias, y
    d.N, d.H, d.W, d.C, d.x_cstride = n, h, wd, c, x_cstride
    d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w = kh, kw, ph, pw, sh, sw
    d.OH = (h + 2 * ph - (dilation * (kh - 1) + 1)) // sh + 1
    d.OW = (wd + 2 * pw - (dilation * (kw - 1) + 1)) // sw + 1
    d.y_cstride, d.y_coffset, d.flags, d.dilation = y_cstride, y_coffset, flags, dilation
    return d


class SolverSeg(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("count", C.c_uint64), ("lr_mult", C.c_float), ("decay_mult", C.c_float)]


class LayoutDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p)] + [(k, C.c_int32) for k in ("N", "C", "H", "W", "src_cstride", "src_coffset")]


class PoolDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("idx", C.c_void_p)] + [(k, C.c_int32) for k in (
        "N", "H", "W", "C", "x_cstride", "k", "stride", "pad", "OH", "OW", "y_cstride", "y_coffset", "f16")]


class SceneObj(C.Structure):
    _fields_ = [("img", C.c_void_p), ("mask", C.c_void_p)] + [(k, C.c_int32) for k in (
        "src_h", "src_w", "flip", "roi_x", "roi_y", "roi_w", "roi_h", "out_w", "out_h", "cx", "cy", "label1")]


class ColorParams(C.Structure):
    _fields_ = [("sharpen_centre", C.c_float), ("sharpen_off", C.c_float), ("add", C.c_int32 * 3), ("mul", C.c_float * 3),
                ("gray_alpha", C.c_float), ("gray_keep", C.c_float)]


GAUSS_MAX_RADIUS = 15
REPLICA_STREAMS = 4            # FCN_REPLICA_STREAMS


class FlipSeg(C.Structure):
    _fields_ = [("w_offset", C.c_uint64), ("wt_offset", C.c_uint64), ("Cout", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
                ("Cin", C.c_int32), ("Cin4", C.c_int32), ("Cout4", C.c_int32)]


class DetectParams(C.Structure):
    _fields_ = [
        ("num_classes", C.c_int32), ("gy", C.c_int32), ("gx", C.c_int32), ("cell_w", C.c_int32), ("cell_h", C.c_int32),
        ("cvg_cstride", C.c_int32), ("cvg_coffset", C.c_int32), ("box_cstride", C.c_int32), ("box_coffset", C.c_int32),
        ("prob_thresh", C.c_float), ("group_thresh", C.c_int32), ("eps", C.c_double), ("min_height", C.c_int32),
        ("round_mode", C.c_int32), ("max_out", C.c_int32),
    ]


class SsdHead(C.Structure):
    """fcn_ssd_head: one head of the Permute + Flatten + Concat gather."""
    _fields_ = [("src", C.c_void_p)] + [(k, C.c_int32) for k in ("pixels", "C", "cstride", "coffset", "dst_col", "reserved")]


class DetOutParams(C.Structure):
    """fcn_detout_params: DetectionOutput."""
    _fields_ = [(k, C.c_int32) for k in ("N", "P", "num_classes", "background", "code_type", "variance_encoded", "top_k", "keep_top_k")] + [
        ("conf_threshold", C.c_float), ("nms_threshold", C.c_float)] + [(k, C.c_int32) for k in ("loc_rstride", "conf_rstride", "capacity", "reserved")]


class ProposalParams(C.Structure):
    """fcn_proposal_params: Proposal."""
    _fields_ = [(k, C.c_int32) for k in ("H", "W", "A", "feat_stride", "pre_nms_topn", "post_nms_topn")] + [
        ("min_size", C.c_float), ("nms_thresh", C.c_float)] + [(k, C.c_int32) for k in (
            "score_cstride", "score_coffset", "delta_cstride", "delta_coffset", "rois_cstride", "rois_coffset", "top_score_cstride",
            "top_score_coffset")] + [("anchors", C.c_float * 128)]


PROPOSAL_MAX_ANCHORS = 32      # FCN_PROPOSAL_MAX_ANCHORS
PROPOSAL_MAX_CANDIDATES = 65536    # FCN_PROPOSAL_MAX_CANDIDATES
PROPOSAL_MAX_PRE_NMS = 6144    # FCN_PROPOSAL_MAX_PRE_NMS
SSD_MAX_HEADS = 16             # FCN_SSD_MAX_HEADS
DETOUT_MAX_TOPK = 1024         # FCN_DETOUT_MAX_TOPK
CODE_CORNER, CODE_CENTER_SIZE = 1, 2
CONV_RELU, CONV_SIGMOID2, CONV_ACCUM, CONV_OUT_F32, CONV_F16, CONV_OUT_F16, CONV_MASK = 1, 2, 4, 8, 16, 32, 64
IP_MAX_ROWS = 32               # FCN_IP_MAX_ROWS: rows the InnerProduct streaming kernels take
IP_WEIGHTS_NT = 256            # FCN_IP_WEIGHTS_NT


def ip_rows_refusal(layer: str, rows: int) -> str:
    """What both engines and the backward planner say of an InnerProduct above IP_MAX_ROWS rows in a NetSpec built without ip_gemm=True."""
    return ("InnerProduct %s: a batch of %d rows (the streaming kernels take at most %d): the matrix-core kernels take any row count for "
            "a NetSpec built with ip_gemm=True (caffe.Net, the solvers and the caffe tool pass it)" % (layer, rows, IP_MAX_ROWS))
CONV_IMAGE_ONES = 128      # half image whose channels 3 and 4 are the constant 1 (the folded Power shift): see include/fcnhip.h
ELT_PROD, ELT_SUM, ELT_MAX = 0, 1, 2
ARGMAX_MAX_TOPK = 32           # FCN_ARGMAX_MAX_TOPK
ACT_PRELU, ACT_TANH, ACT_BIAS = 0, 1, 2      # FCN_ACT_*: the modes of csrc/act.hip
ACT_MODES = {"PReLU": ACT_PRELU, "TanH": ACT_TANH, "Bias": ACT_BIAS}
NEURON_ELU, NEURON_CLIP, NEURON_ABSVAL, NEURON_BNLL, NEURON_SWISH = 0, 1, 2, 3, 4      # FCN_NEURON_*: the modes of csrc/neuron.hip
NEURON_MODES = {"ELU": NEURON_ELU, "ReLU6": NEURON_CLIP, "Clip": NEURON_CLIP, "AbsVal": NEURON_ABSVAL, "BNLL": NEURON_BNLL, "Swish": NEURON_SWISH}
ARGMAX_WAVE_BYTES, ARGMAX_WAVE_PIXELS, ARGMAX_WAVE_MIN_C = 512, 8192, 32      # FCN_ARGMAX_WAVE_*: where a wave takes a pixel (csrc/argmax.hip)
ARGMAX_VALUES, ARGMAX_PAIRS, ARGMAX_SOFTMAX = 1, 2, 4
SOLVER_KINDS = {"SGD": 0, "NESTEROV": 1, "ADAGRAD": 2, "RMSPROP": 3, "ADADELTA": 4, "ADAM": 5}      # FCN_SOLVER_*
REG_L2, REG_L1 = 0, 1
RECT_ROUND_NEAREST_EVEN, RECT_ROUND_TRUNCATE = 0, 1

_vp, _i, _f, _d, _sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t

# name -> (restype, argtypes).  Every symbol include/fcnhip.h declares is listed here.
PROTOTYPES = {
    "fcn_abi_version": (_i, []),
    "fcn_last_error_string": (C.c_char_p, []),
    "fcn_device_count": (_i, [C.POINTER(_i)]),
    "fcn_init": (_i, [_i]),
    "fcn_device_name": (_i, [C.c_char_p, _i]),
    "fcn_device_sync": (_i, []),
    "fcn_malloc": (_i, [C.POINTER(_vp), _sz]),
    "fcn_free": (_i, [_vp]),
    "fcn_host_malloc": (_i, [C.POINTER(_vp), _sz]),
    "fcn_host_free": (_i, [_vp]),
    "fcn_memset_async": (_i, [_vp, _i, _sz, _vp]),
    "fcn_memcpy_h2d_async": (_i, [_vp, _vp, _sz, _vp]),
    "fcn_memcpy_d2h_async": (_i, [_vp, _vp, _sz, _vp]),
    "fcn_memcpy_d2d_async": (_i, [_vp, _vp, _sz, _vp]),
    "fcn_stream_create": (_i, [C.POINTER(_vp)]),
    "fcn_stream_destroy": (_i, [_vp]),
    "fcn_stream_sync": (_i, [_vp]),
    "fcn_event_create": (_i, [C.POINTER(_vp)]),
    "fcn_event_destroy": (_i, [_vp]),
    "fcn_event_record": (_i, [_vp, _vp]),
    "fcn_event_sync": (_i, [_vp]),
    "fcn_event_elapsed_ms": (_i, [_vp, _vp, C.POINTER(_f)]),
    "fcn_graph_begin": (_i, [_vp]),
    "fcn_graph_end": (_i, [_vp, C.POINTER(_vp)]),
    "fcn_graph_launch": (_i, [_vp, _vp]),
    "fcn_graph_destroy": (_i, [_vp]),
    "fcn_stream_create_replica": (_i, [C.POINTER(_vp), _i]),
    "fcn_stream_is_prioritized": (_i, [_vp, C.POINTER(_i)]),
    "fcn_nchw_to_nhwc_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "fcn_nhwc_to_nchw_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "fcn_nhwc_to_nchw_multi_f32": (_i, [C.POINTER(LayoutDesc), _i, _vp]),
    "fcn_conv2d_fwd_f32": (_i, [C.POINTER(ConvDesc), _vp]),
    "fcn_conv2d_group_workspace_bytes": (_sz, [_i]),
    "fcn_conv2d_num_configs": (_i, []),
    "fcn_conv2d_first_layer_config": (_i, []),
    "fcn_conv2d_config_lds_bytes": (_i, [_i]),
    "fcn_conv2d_config_waves_k": (_i, [_i]),
    "fcn_conv2d_group_prepare": (_i, [C.POINTER(ConvDesc), _i, _vp, _i, C.POINTER(ConvGroup)]),
    "fcn_conv2d_group_prepare_fused": (_i, [C.POINTER(ConvDesc), _i, C.POINTER(PoolDesc), _i, _vp, _i, C.POINTER(ConvGroup)]),
    "fcn_conv2d_fwd_group_f32": (_i, [C.POINTER(ConvGroup), _vp]),
    "fcn_conv2d_group_release": (_i, [_vp]),
    "fcn_conv2d_tail_scratch_bytes": (C.c_size_t, [C.POINTER(ConvTail)]),
    "fcn_conv2d_tail_arrive_bytes": (C.c_size_t, [C.POINTER(ConvTail)]),
    "fcn_conv2d_group_attach_tail": (_i, [_vp, C.POINTER(ConvTail)]),
    "fcn_maxpool_fwd_f32": (_i, [_vp, _vp, _vp] + [_i] * 12 + [_vp]),
    "fcn_avepool_fwd_f32": (_i, [_vp, _vp] + [_i] * 12 + [_vp]),
    "fcn_lrn_fwd_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _vp]),
    "fcn_maxpool_lrn5_fwd_f32": (_i, [_vp, _vp] + [_i] * 12 + [_f, _f, _f, _vp]),
    "fcn_maxpool_lrn5_fwd_f16": (_i, [_vp, _vp] + [_i] * 12 + [_f, _f, _f, _vp]),
    "fcn_maxpool_lrn5_conv1x1_fwd_f32": (_i, [_vp] + [_i] * 10 + [_f, _f, _f, _vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    "fcn_maxpool_lrn5_conv1x1_fwd_f16": (_i, [_vp] + [_i] * 10 + [_f, _f, _f, _vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    "fcn_relu_fwd_f32": (_i, [_vp, _vp, _sz, _f, _vp]),
    "fcn_sigmoid_fwd_f32": (_i, [_vp, _vp, _sz, _vp]),
    "fcn_power_fwd_f32": (_i, [_vp, _vp, _sz, _f, _f, _f, _vp]),
    "fcn_eltwise_fwd_f32": (_i, [_vp, _vp, _vp, _sz, _i, _f, _f, _vp]),
    "fcn_copy_channels_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "fcn_deconv_depthwise_fwd_f32": (_i, [_vp, _vp, _vp, _vp] + [_i] * 12 + [_vp]),
    "fcn_preprocess_bgr8": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _f, _vp, _vp]),
    "fcn_detect_workspace_bytes": (_sz, [C.POINTER(DetectParams), _i]),
    "fcn_detect_decode_group": (_i, [_vp, _vp, _i, _sz, _sz, C.POINTER(DetectParams), _vp, _vp, _vp, _vp, _vp]),
    "fcn_score_masks_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "fcn_score_masks": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _f, _vp, _i, _i, _vp, _vp, _vp]),
    "fcn_gen_targets": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fcn_gen_targets_nhwc": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _d, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "fcn_conv2d_wgrad_workspace_floats": (_sz, [C.POINTER(ConvDesc), C.POINTER(_i)]),
    "fcn_conv2d_wgrad_f32": (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp]),
    "fcn_conv2d_wgrad_group_workspace_floats": (_sz, [C.POINTER(ConvDesc), _i]),
    "fcn_conv2d_wgrad_group_f32": (_i, [C.POINTER(ConvDesc), _vp, _vp, _i, _vp, _vp]),
    "fcn_conv2d_wgrad_num_configs": (_i, []),
    "fcn_conv2d_wgrad_split_config": (_i, []),
    "fcn_conv2d_wgrad_workspace_floats_cfg": (_sz, [C.POINTER(ConvDesc), _i, C.POINTER(_i)]),
    "fcn_conv2d_wgrad_cfg_f32": (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _i, _vp]),
    "fcn_conv2d_wgrad_group_workspace_floats_cfg": (_sz, [C.POINTER(ConvDesc), _i, _i]),
    "fcn_conv2d_wgrad_group_cfg_f32": (_i, [C.POINTER(ConvDesc), _vp, _vp, _i, _vp, _i, _vp]),
    "fcn_conv_weights_flip_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "fcn_nchw_f32_to_nhwc_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "fcn_nhwc_f16_to_nchw_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "fcn_maxpool_fwd_f16": (_i, [_vp, _vp] + [_i] * 12 + [_vp]),
    "fcn_lrn_fwd_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _vp]),
    "fcn_avepool_fwd_f16": (_i, [_vp, _vp] + [_i] * 12 + [_vp]),
    "fcn_deconv_depthwise_fwd_f16": (_i, [_vp, _vp, _vp, _vp] + [_i] * 13 + [_vp]),
    "fcn_eltwise_fwd_f16": (_i, [_vp, _vp, _vp, _sz, _i, _f, _f, _vp]),
    "fcn_softmax_fwd_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "fcn_copy_channels_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "fcn_preprocess_bgr8_batch": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _i, _f, _vp, _vp]),
    "fcn_preprocess_bgr8_rois": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _f, _vp, _vp]),
    "fcn_preprocess_bgr8_f16": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _f, _vp, _vp]),
    "fcn_compose_scene_bgr8": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _i, _i, _vp]),
    "fcn_mask_to_label_f32": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _vp]),
    "fcn_compose_scene_view_bgr8": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "fcn_blur_gauss_bgr8": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp]),
    "fcn_blur_box_bgr8": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "fcn_blur_median_bgr8": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "fcn_color_augment_bgr8": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "fcn_softmax_fwd_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "fcn_softmax_loss_workspace_bytes": (_sz, []),
    "fcn_softmax_loss_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "fcn_deconv_depthwise_bwd_f32": (_i, [_vp, _vp, _vp] + [_i] * 13 + [_vp]),
    "fcn_conv_weights_flip_batch_f32": (_i, [_vp, _vp, _vp, _i, _vp]),
    "fcn_relu_bwd_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "fcn_relu_bwd_slope_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _i, _vp]),
    "fcn_sigmoid_bwd_f32": (_i, [_vp, _vp, _vp, _sz, _i, _vp]),
    "fcn_maxpool_bwd_f32": (_i, [_vp, _vp, _vp] + [_i] * 14 + [_vp]),
    "fcn_maxpool_bwd_mask_f32": (_i, [_vp, _vp, _vp] + [_i] * 14 + [_vp, _i, _i, _vp]),
    "fcn_avepool_bwd_f32": (_i, [_vp, _vp] + [_i] * 14 + [_vp]),
    "fcn_lrn_bwd_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _i, _vp]),
    "fcn_dropout_f32": (_i, [_vp, _vp] + [_i] * 8 + [_f, C.c_uint, C.c_uint, _vp]),
    "fcn_stream_wait_event": (_i, [_vp, _vp]),
    "fcn_comm_unique_id": (_i, [C.c_char_p]),
    "fcn_comm_init": (_i, [C.POINTER(_vp), C.c_char_p, _i, _i]),
    "fcn_comm_allreduce_sum_f32": (_i, [_vp, _vp, _sz, _vp]),
    "fcn_comm_destroy": (_i, [_vp]),
    "fcn_loss_f32": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "fcn_sgd_update_f32": (_i, [_vp, _vp, _vp, _vp, _i, _f, _f, _f, _f, _vp]),
    "fcn_adam_update_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _f, _f, _i, _f, _vp]),
    "fcn_solver_update_f32": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _f, _f, _f, _i, _i, _f, _vp, _vp]),
    "fcn_grad_clip_workspace_bytes": (_sz, []),
    "fcn_grad_clip_f32": (_i, [_vp, _vp, _i, _f, _f, _vp, _vp, _vp, _vp]),
    "fcn_grad_accumulate_f32": (_i, [_vp, _vp, _sz, _i, _vp]),
    "fcn_score_accumulate_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "fcn_accuracy_workspace_bytes": (_sz, []),
    "fcn_accuracy_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "fcn_tconv2d_num_configs": (_i, []),
    "fcn_tconv2d_workspace_bytes": (_sz, [C.POINTER(TConvDesc), _i]),
    "fcn_tconv2d_prepare": (_i, [C.POINTER(TConvDesc), _i, _vp, _i, C.POINTER(TConvPlan)]),
    "fcn_tconv2d_f32": (_i, [C.POINTER(TConvPlan), _vp]),
    "fcn_tconv_bank_floats": (_sz, [_i, _i, _i, _i]),
    "fcn_tconv_bank_pack_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "fcn_tconv2d_num_configs_f16": (_i, []),
    "fcn_tconv2d_prepare_f16": (_i, [C.POINTER(TConvDesc), _i, _vp, _i, C.POINTER(TConvPlan)]),
    "fcn_tconv2d_f16": (_i, [C.POINTER(TConvPlan), _vp]),
    "fcn_tconv_bank_halves": (_sz, [_i, _i, _i, _i]),
    "fcn_tconv_bank_pack_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "fcn_channel_sum_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "fcn_rconv2d_num_configs": (_i, []),
    "fcn_rconv2d_workspace_bytes": (_sz, [C.POINTER(RConvDesc), _i]),
    "fcn_rconv2d_prepare": (_i, [C.POINTER(RConvDesc), _i, _vp, _i, C.POINTER(RConvPlan)]),
    "fcn_rconv2d_f32": (_i, [C.POINTER(RConvPlan), _vp]),
    "fcn_rconv2d_num_configs_f16": (_i, []),
    "fcn_rconv2d_prepare_f16": (_i, [C.POINTER(RConvDesc), _i, _vp, _i, C.POINTER(RConvPlan)]),
    "fcn_rconv2d_f16": (_i, [C.POINTER(RConvPlan), _vp]),
    "fcn_rconv2d_wgrad_workspace_floats": (_sz, [C.POINTER(RConvDesc)]),
    "fcn_rconv2d_wgrad_f32": (_i, [C.POINTER(RConvDesc), _vp, _vp, _vp, _vp]),
    "fcn_dwconv2d_num_configs": (_i, []),
    "fcn_dwconv2d_fwd_f32": (_i, [C.POINTER(DwConvDesc), _i, _vp]),
    "fcn_dwconv2d_fwd_f16": (_i, [C.POINTER(DwConvDesc), _i, _vp]),
    "fcn_dwconv2d_dgrad_f32": (_i, [C.POINTER(DwConvDesc), _i, _vp]),
    "fcn_dwconv2d_wgrad_workspace_floats": (_sz, [C.POINTER(DwConvDesc), _i]),
    "fcn_dwconv2d_wgrad_f32": (_i, [C.POINTER(DwConvDesc), _vp, _vp, _vp, _i, _vp]),
    "fcn_crop_fwd_f32": (_i, [_vp, _vp] + [_i] * 12 + [_vp]),
    "fcn_crop_fwd_f16": (_i, [_vp, _vp] + [_i] * 12 + [_vp]),
    "fcn_crop_fwd_f16_f32": (_i, [_vp, _vp] + [_i] * 12 + [_vp]),
    "fcn_crop_bwd_f32": (_i, [_vp, _vp] + [_i] * 13 + [_vp]),
    "fcn_interp_fwd_f32": (_i, [_vp, _vp] + [_i] * 12 + [_vp]),
    "fcn_interp_fwd_f16": (_i, [_vp, _vp] + [_i] * 13 + [_vp]),
    "fcn_interp_bwd_f32": (_i, [_vp, _vp] + [_i] * 13 + [_vp]),
    "fcn_argmax_fwd_f32": (_i, [_vp, _vp] + [_i] * 8 + [_vp]),
    "fcn_argmax_fwd_f16": (_i, [_vp, _vp] + [_i] * 8 + [_vp]),
    "fcn_interp_argmax_fwd_f32": (_i, [_vp, _vp] + [_i] * 13 + [_vp]),
    "fcn_interp_argmax_fwd_f16": (_i, [_vp, _vp] + [_i] * 13 + [_vp]),
    "fcn_unpool_fwd_f32": (_i, [_vp, _vp, _vp] + [_i] * 13 + [_vp]),
    "fcn_unpool_fwd_f16": (_i, [_vp, _vp, _vp] + [_i] * 14 + [_vp]),
    "fcn_unpool_bwd_f32": (_i, [_vp, _vp, _vp] + [_i] * 14 + [_vp]),
    "fcn_maxpool_idx_fwd_f16": (_i, [_vp, _vp, _vp] + [_i] * 12 + [_vp]),
    "fcn_pool_mask_to_nchw_f32": (_i, [_vp, _vp] + [_i] * 4 + [_vp]),
    "fcn_inner_product_workspace_bytes": (_sz, [_i, _i, _i]),
    "fcn_inner_product_fwd_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "fcn_inner_product_fwd_f32": (_i, [_vp, _i, _vp, _vp, _vp] + [_i] * 6 + [_vp, _vp]),
    "fcn_inner_product_fwd_f16": (_i, [_vp, _i, _vp, _vp, _vp] + [_i] * 6 + [_vp, _vp]),
    "fcn_inner_product_bwd_data_f32": (_i, [_vp, _i, _i, _vp, _vp] + [_i] * 5 + [_vp, _vp]),
    "fcn_inner_product_bwd_weights_f32": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp] + [_i] * 4 + [_vp]),
    "fcn_ip_gemm_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "fcn_ip_gemm_fwd_f32": (_i, [_vp, _i, _vp, _vp, _vp] + [_i] * 6 + [_vp, _vp]),
    "fcn_ip_gemm_fwd_f16": (_i, [_vp, _i, _vp, _vp, _vp] + [_i] * 6 + [_vp, _vp]),
    "fcn_ip_gemm_bwd_data_f32": (_i, [_vp, _i, _i, _vp, _vp] + [_i] * 5 + [_vp, _vp]),
    "fcn_ip_gemm_bwd_weights_f32": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp] + [_i] * 4 + [_vp, _vp]),
    "fcn_batchnorm_workspace_bytes": (_sz, [_i, _i]),
    "fcn_batchnorm_stats_f32": (_i, [_vp] + [_i] * 4 + [_vp, _vp, _vp, _f, _f, _vp, _vp, _vp]),
    "fcn_batchnorm_apply_f32": (_i, [_vp, _vp, _vp] + [_i] * 7 + [_vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _vp]),
    "fcn_batchnorm_apply_f16": (_i, [_vp, _vp] + [_i] * 6 + [_vp, _vp, _vp, _f, _vp, _vp, _i, _vp]),
    "fcn_batchnorm_bwd_reduce_f32": (_i, [_vp, _vp, _vp] + [_i] * 8 + [_vp, _vp, _vp, _vp]),
    "fcn_batchnorm_bwd_apply_f32": (_i, [_vp, _vp, _vp, _vp] + [_i] * 10 + [_vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _vp]),
    "fcn_scale_gate_workspace_bytes": (_sz, [_i, _i, _i]),
    "fcn_scale_gate_fwd_f32": (_i, [_vp, _vp, _vp, _vp] + [_i] * 11 + [_vp]),
    "fcn_scale_gate_fwd_f16": (_i, [_vp, _vp, _vp, _vp] + [_i] * 11 + [_vp]),
    "fcn_scale_gate_bwd_data_f32": (_i, [_vp, _vp, _vp] + [_i] * 9 + [_vp]),
    "fcn_scale_gate_bwd_gate_f32": (_i, [_vp, _vp, _vp] + [_i] * 9 + [_vp, _vp]),
    "fcn_act_workspace_bytes": (_sz, [_i, _i]),
    "fcn_act_fwd_f32": (_i, [_vp, _vp, _vp] + [_i] * 8 + [_vp, _i, _vp]),
    "fcn_act_fwd_f16": (_i, [_vp, _vp] + [_i] * 7 + [_vp, _i, _vp]),
    "fcn_act_bwd_data_f32": (_i, [_vp, _vp, _vp] + [_i] * 9 + [_vp, _i, _i, _vp]),
    "fcn_act_bwd_param_f32": (_i, [_vp, _vp, _vp] + [_i] * 8 + [_vp, _vp]),
    "fcn_neuron_fwd_f32": (_i, [_vp, _vp, _vp] + [_i] * 8 + [_f, _f, _vp]),
    "fcn_neuron_fwd_f16": (_i, [_vp, _vp] + [_i] * 7 + [_f, _f, _vp]),
    "fcn_neuron_bwd_f32": (_i, [_vp, _vp, _vp] + [_i] * 9 + [_f, _f, _i, _vp]),
    "fcn_shuffle_channel_f32": (_i, [_vp, _vp] + [_i] * 8 + [_vp]),
    "fcn_shuffle_channel_f16": (_i, [_vp, _vp] + [_i] * 7 + [_vp]),
    "fcn_ssd_gather_f32": (_i, [C.POINTER(SsdHead), _i, _i, _vp, _i, _i, _vp]),
    "fcn_normalize_fwd_f32": (_i, [_vp, _vp, _vp] + [_i] * 7 + [_f, _vp]),
    "fcn_detection_output_workspace_bytes": (_sz, [C.POINTER(DetOutParams)]),
    "fcn_detection_output_f32": (_i, [_vp, _vp, _vp, C.POINTER(DetOutParams), _vp, _vp, _vp, _sz, _vp]),
    "fcn_pair_softmax_f32": (_i, [_vp, _vp] + [_i] * 6 + [_vp]),
    "fcn_proposal_workspace_bytes": (_sz, [C.POINTER(ProposalParams)]),
    "fcn_proposal_f32": (_i, [_vp, _vp, _vp, C.POINTER(ProposalParams), _vp, _vp, _vp, _vp, _sz, _vp]),
    "fcn_roi_pool_fwd_f32": (_i, [_vp, _vp, _vp, _vp] + [_i] * 11 + [_f, _i, _i, _vp]),
    "fcn_psroi_pool_fwd_f32": (_i, [_vp, _vp, _vp] + [_i] * 11 + [_f, _i, _i, _vp]),
}

HW_QUEUES: dict = {}      # what load() found / did about GPU_MAX_HW_QUEUES
_lib: Optional[C.CDLL] = None
_lock = threading.Lock()


def load() -> C.CDLL:
    """Load libfcnhip.so (once) and attach prototypes.  Raises loudly when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.isfile(LIB_PATH):
            raise FcnLibraryError(
                "libfcnhip.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C fcn_object_detector_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        # The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), in creation
        # order and counting idle streams; it reads the variable once, when it initialises.  Streams that share a queue do
        # not overlap: with 4 queues a fourth replica stream of a frame pipeline aliases another one and throughput DROPS
        # (3460 vs 4300 frames/s), the two-stream training step runs 6.60 vs 6.37 ms; with 8 the node pipeline lost a third
        # of its rate as soon as another pipeline's four idle streams existed (2590 vs 3600 frames/s).  16 covers the
        # engines a process of this package keeps alive at once; no measured cost against 8.  (The frame pipelines' replicas no
        # longer depend on this: fcn_stream_create_replica takes their queues from the pool of another stream priority, which the
        # default limit of 4 covers.  Plain streams - the training step's two, lone engines - are what the 16 still serves.)
        # An embedding process should export GPU_MAX_HW_QUEUES itself; the variable is only filled in
        # here when nobody has set it and $FCN_SET_HW_QUEUES is not 0 - and that is said once, not done silently.
        global HW_QUEUES
        if "GPU_MAX_HW_QUEUES" in os.environ:
            HW_QUEUES = {"value": os.environ["GPU_MAX_HW_QUEUES"], "set_by": "environment"}
        elif os.environ.get("FCN_SET_HW_QUEUES", "1") != "0":
            os.environ["GPU_MAX_HW_QUEUES"] = "16"
            HW_QUEUES = {"value": "16", "set_by": "fcn_object_detector_amd.lib.load"}
            if os.environ.get("FCN_QUIET", "0") in ("", "0"):
                import sys
                sys.stderr.write("fcn_object_detector_amd: GPU_MAX_HW_QUEUES was unset; set to 16 for this process (export it yourself or "
                                 "FCN_SET_HW_QUEUES=0 to keep the runtime's default; FCN_QUIET=1 silences this line)\n")
        else:
            HW_QUEUES = {"value": None, "set_by": "nobody (FCN_SET_HW_QUEUES=0): the HIP runtime's default of 4 applies"}
        # RCCL's intra-node transport shares buffers between rank processes through dmabuf IPC; on hosts whose driver only
        # supports that mode the legacy handle path fails with `hipIpcGetMemHandle: invalid argument`.  Read by the HSA
        # runtime when it initialises, so it is filled in here for ranks that a foreign launcher (torch.distributed.run)
        # started without it - only when the job has more than one rank and nobody has set it.
        if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        try:
            lib = C.CDLL(LIB_PATH, mode=C.RTLD_LOCAL)
        except OSError as e:  # pragma: no cover - depends on the box
            raise FcnLibraryError("cannot load %s: %s" % (LIB_PATH, e)) from e
        for name, (res, args) in PROTOTYPES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise FcnLibraryError("libfcnhip.so lacks symbol %s (stale build?)" % name) from e
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def substitute(obj):
    """Put `obj` in the loaded library's place (what load() returns) and return what was there: tools that time or count the
    library's calls wrap the real object and hand it back when they are done (tools/frame_path.py)."""
    global _lib
    load()
    prev, _lib = _lib, obj
    return prev


def check(rc: int) -> None:
    if rc != 0:
        msg = load().fcn_last_error_string()
        raise FcnError(rc, msg.decode("utf-8", "replace") if msg else "")


def call(name: str, *args) -> None:
    """Call an int-returning entry point and raise :class:`FcnError` on a non-zero code."""
    check(getattr(load(), name)(*args))
