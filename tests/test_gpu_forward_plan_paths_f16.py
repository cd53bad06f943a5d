"""The half-float forward planner's storage and fusion paths, one tiny net per path, every blob against float64 rounded where the engine rounds.

The twin of tests/test_gpu_forward_plan_paths.py for Engine(dtype="f16"), with that module's prototxt helpers, Case and Wrong.  Every case
is a few layers over `data` (2 x C x 11 x 10, C = 8 or 16, 3 or 4 for the image cases; 1 x 8 x 128 x 128 and 1 x 8 x 256 x 256 where a size
decides the path), run as Engine(NetSpec(msg), params=..., device=0, autotune=False, dtype="f16") with seeded parameters and inputs.  A
case states, and the GPU test asserts exactly, (1) the plan: the launch list as (kind, label) pairs, eng.alias, eng.shift,
eng.copy_concats, eng.copy_slices, eng._conv_layer_meta, the keys of eng._lazy_blob_ops, the element size of every blob, eng._half_inputs
and - where the case names them - the CONV_F16 / CONV_OUT_F32 / CONV_OUT_F16 / CONV_IMAGE_ONES flags of the convolution descriptors;
(2) every blob through eng.read_blob against the rounded reference, the lazy blobs once ahead of the others and once behind them;
(3) identical bits of all outputs from forward() twice, from a forward() behind the lazy reads and from forward(use_graph=False).  (2) is
repeated with fuse=False, group_convs=False and with fuse=True, group_convs=False, each against the reference rounded for that plan.

The reference is tests/torch_forward_ref.forward_net in float64 with two hooks (rounding_hooks below states the rules):
  store      rounds to the nearest half every blob that storage.plan_blobs(spec, shapes, inputs, outputs, True, fuse, half_image).esize lays
             out in 2-byte elements, each time a layer writes it - but for the writes a case lists in `raw`, which a fused launch keeps in
             registers (the middles of BatchNorm -> Scale -> ReLU; the middle of Pool -> LRN and LRN -> Pool, where it changes nothing: a
             test below holds that the maximum of rounded values is the rounded maximum).  An Eltwise over three bottoms is two launches
             and rounds its partial result.  An input reads back as the host array it was uploaded from.
  operands   storage.param_layout's rule: the filters of a Convolution or InnerProduct are halves when its bottom holds halves; biases, the
             filters of a depthwise Convolution (always float32) and of a depthwise Deconvolution, BatchNorm and Scale blobs, and the first
             layer's filters under a float32 image stay float32.  Behind a half image the convolution reads the un-shifted halves and two
             channels of ones, and its filters carry the shift times the sum of the ROUNDED filters per tap as a half plus the half of the
             remainder, as storage.pack builds them.

The matrix:
  A  element types  Convolution float32 input -> halves -> halves -> float32 output; Convolution of halves with a Sigmoid second top (both
                    tops float32, one launch); InnerProduct halves -> halves with a fused ReLU -> float32; depthwise Convolution halves ->
                    halves -> float32; Softmax, depthwise Deconvolution, Interp and Upsample each as a half middle blob and as a float32
                    output (the Upsample case is also D's masked pooling of halves, its masks read back).
  B  half image     data (3 channels) -> Power(shift -127) -> padded 3 x 3 convolution, and 5 x 5 / stride 2: half_inputs taken,
                    CONV_IMAGE_ONES set (the input stride is 8), data reads back un-shifted and the Power top shifted; with filters whose
                    taps sum to zero; with FCN_F16_IMAGE=0 (float32 upload with the shift folded in); with fuse=False (a Power launch).
                    The fold is not taken, and the float32 path is, for scale 2, a second reader of the Power top, the Power top as an
                    output (the convolution then reads `data`: a blob no layer reads is the only kind of output), a depthwise first layer
                    and a 4-channel input.
  C  views          Concat of two 8-channel tops (a view), of a 4- and a 12-channel member (copies; a view in float32), with a Pooling
                    member carrying an in-place ReLU (fcn_batchnorm_apply_f16 on the window), with an in-place Dropout member; Slice at 8
                    (views) and at 4 (copies); a Slice of a Concat view; Dropout to another top (alias); Crop of halves.
  D  pool / LRN     Pool -> LRN and LRN -> Pool as single launches with a lazy middle; Pool(3, 2) -> LRN(5) -> 1 x 1 Convolution 64 -> 64 +
                    ReLU as one launch at 1 x 64 x 256 x 256 - in halves that launch is taken from 2^22 elements on - and as Pool + LRN and a
                    convolution launch below that size; the two-launch plans for a second consumer and a mask top; MAX, AVE and global AVE
                    and MAX pooling launched alone; a MAX pooling riding in a convolution launch below 16384 pixels and launching alone at
                    16384.
  E  BatchNorm      BatchNorm -> Scale -> ReLU with global statistics in place and with separate tops (lazy middles), cut by a second
                    consumer; Eltwise SUM with coefficients, PROD and MAX over three half bottoms; a ReLU of its own on an Eltwise top, and
                    behind a convolution whose top has an earlier reader (the reader sees the values ahead of the ReLU).
  F  levels         3 x 3 and 1 x 1 convolutions of halves in one group launch; group: 2 with 8-channel output groups; FCN_CONV_TAIL=1
                    beside the same net without it: the same plan (the tail is float32 only).
  G  refusals       by exception type and message.  Without a GPU, from storage.plan_blobs / param_layout: SSD heads, region layers, a
                    float32 blob produced by a Pooling, a view of a root with another element size, Deconvolution with group 1.  On the GPU,
                    from the engine: TRAIN phase, dilated and rectangular Convolution, Accuracy, a leaky ReLU over halves, LRN with
                    local_size 3 or over 12 channels, MAX pooling over 12 channels, BatchNorm with batch statistics, Eltwise / Concat copy /
                    Crop / Scale chain / InnerProduct / Interp / Upsample between half and float32 blobs, a grouped Convolution whose
                    output groups split an 8-half segment.
What could not be built as a case of A - F: "LRN with local_size 3 as a two-launch plan" - the half LRN kernel takes local_size 5 only.
The engine used to plan such a net and fail at the first forward, inside the graph capture; it now refuses it when it plans, and the net
is a case of G.  "A lazy middle blob as a net output" is no case for the reason the float32 module gives; the part without a GPU holds it.

The part without a GPU shows on the reference alone that each case CAN fail: Case.wrong names one wrong evaluation (two 4-channel runs of a
Concat member swapped, members swapped, a lazy middle at its zero fill, the shift applied twice on read-back or not at all, the shift
added inside the zero padding, the image rounded to halves after the shift, a float32 output rounded to halves - with filters scaled so
that it leaves the half range: an output rounded inside the range moves by 2^-11 of itself, under any threshold above float32 noise, and
what holds that path is the exact assertion of CONV_OUT_F32 and of the blob's element size -, a Sigmoid top without its Sigmoid, an
Upsample that ignores the mask, batch statistics for global ones, an Eltwise coefficient dropped, ...) that must be at least 10 x TOL away in rel_err on a blob the GPU test compares.  The inputs
are held to what the float32 module holds them to: a tenth of what every ReLU reads on each side of zero, no MAX pooling window with a
tie among the ROUNDED values - but at 128 x 128 and 256 x 256, where some of the 10^5 windows of halves always tie (71 and 608 do); those
poolings write no mask, and the maximum of tied values is that value; the part without a GPU holds that an exempt pooling has one top.

Thresholds, measured and not chosen.  The kernels accumulate in float32 from the operands the reference rounds, so they differ from it by
float32 noise and by the halves that noise pushes across a rounding boundary, one half ulp each, which then travel downstream.  The
float32 run of the interpreter with the same hooks against the float64 one, over every case, both plans and three seeds:
    worst rel_err                                      7.89e-4  (pool_lrn_conv): MEASURED_F32
    worst elem_err ratio at 2^-10, a first half blob   0.74
    ... behind a computed half blob                    1.58     (pool_lrn_conv): MEASURED_ELEM
    smallest wrong distance                            0.049    (half_image_zero_sum_taps)
TOL = 4 x MEASURED_F32 = 3.16e-3 on rel_err: at most 5e-3, the project's bound for half-float nets, and at most a tenth of 0.049.
Element-wise, conftest.elem_err(.., 2^-10) <= 1 on a blob no computed half blob lies ahead of - one half ulp is at most 2^-10 of the
value, so a single flip passes, and two half ulps fail wherever the value stands above the blob's rms - and <= 4 x MEASURED_ELEM = 6.32
behind one.  The part without a GPU measures again and holds each fresh measurement within a tenth of the recorded value."""
import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import elem_err, rel_err
from fcn_object_detector_amd import proto
from fcn_object_detector_amd import storage as S
from fcn_object_detector_amd.netspec import NetSpec
from test_gpu_forward_plan_paths import (FILL, FUSED, PLAIN, Case, Wrong, bnorm, bottoms, concat, conv, conv1, copies, dropout, elt, fc, launch_list, lrn,
                                         numpy_blobs, pool, power, relu, same_bits, scale, sigmoid, slices, unary, zero)
from torch_forward_ref import forward_net
from torch_resnet_ref import as_torch, random_params

MEASURED_F32 = 7.89e-4                # float32 against float64 interpreter, the worst rel_err as measured
MEASURED_ELEM = 1.58                  # ... the worst elem_err ratio at ELEM_TOL behind a computed half blob, as measured
TOL = 4 * MEASURED_F32                # rel_err of a blob against the rounded reference: 3.16e-3
ELEM_TOL = 2.0 ** -10                 # conftest.elem_err: one half ulp of a value is at most 2^-10 of it
WRONG_AT_LEAST = 10 * TOL
SEEDS = 3
SHIFT = -127.0


# ------------------------------------------------------------------------------------------------------------------ prototxt snippets
def dwconv(name, bottom, n, geometry="kernel_size: 3 pad: 1"):
    return 'layer { name: "%s" type: "DepthwiseConvolution" bottom: "%s" top: "%s" convolution_param { num_output: %d %s %s } }\n' % (
        name, bottom, name, n, geometry, FILL)


def deconv(name, bottom, n, group=None):
    return 'layer { name: "%s" type: "Deconvolution" bottom: "%s" top: "%s" convolution_param { num_output: %d group: %d kernel_size: 4 stride: 2 pad: 1 %s } }\n' % (
        name, bottom, name, n, n if group is None else group, FILL)


def interp(name, bottom, param="zoom_factor: 2"):
    return unary("Interp", name, bottom, name, " interp_param { %s }" % param)


def upsample(name, bottom, mask, h=11, w=10):
    return 'layer { name: "%s" type: "Upsample" bottom: "%s" bottom: "%s" top: "%s" upsample_param { upsample_h: %d upsample_w: %d } }\n' % (name, bottom, mask, name, h, w)


def crop(name, bottom, like, offset=2):
    return 'layer { name: "%s" type: "Crop" bottom: "%s" bottom: "%s" top: "%s" crop_param { axis: 2 offset: %d } }\n' % (name, bottom, like, name, offset)


def softmax(name, bottom):
    return unary("Softmax", name, bottom, name)


def gpool(name, bottom, kind="AVE"):
    return 'layer { name: "%s" type: "Pooling" bottom: "%s" top: "%s" pooling_param { pool: %s global_pooling: true } }\n' % (name, bottom, name, kind)


# ----------------------------------------------------------------------------------------------------------------------- the table
@dataclass(frozen=True)
class HalfCase(Case):
    """A Case of the float32 module plus what the half-float plan adds.  group: the letter of the matrix; f32: the blobs of 4-byte
    elements, complete (every other blob holds halves; a pooling mask is no blob); raw: blob -> the writes (0 = the first layer that
    writes it, 1 = the first in-place layer behind it, ...) whose value a FUSED launch keeps in registers - the next link of the chain
    reads them unrounded; half_image: the data top kept as a half image; flags: Convolution -> CONV_F16 / CONV_OUT_F32 / CONV_OUT_F16 /
    CONV_IMAGE_ONES of its descriptor; env: environment of the engines; engine: keywords of the first engine; shape: of `data`, where it
    is not 2 x c x 11 x 10; tweak: changes the seeded parameters in place; ties: the MAX poolings whose windows hold no tie (None: all)."""
    group: str = "A"
    f32: tuple = ("data",)
    raw: Dict[str, tuple] = field(default_factory=dict)
    half_image: bool = False
    flags: Dict[str, int] = field(default_factory=dict)
    env: Dict[str, str] = field(default_factory=dict)
    engine: Dict[str, bool] = field(default_factory=dict)
    shape: Optional[tuple] = None
    tweak: Optional[Callable] = None
    ties: Optional[tuple] = None

    @property
    def text(self):
        return 'input: "data" input_shape { dim: %d dim: %d dim: %d dim: %d }\n' % (self.shape or (2, self.c, 11, 10)) + self.body


R, F16, OUT32, OUT16, ONES = 1, 16, 8, 32, 128      # lib.CONV_RELU, CONV_F16, CONV_OUT_F32, CONV_OUT_F16, CONV_IMAGE_ONES
C0 = conv("c0", "data", 8)
C12 = conv("c0", "data", 12)      # 12 of the 16 channels of two 8-half segments: the kernels that take any channel count see pad channels


def r16(y):
    return y.to(torch.float16).to(y.dtype)


def scaled(layer, factor):
    def tweak(params):
        params[layer][0] *= np.float32(factor)
        params[layer][1] *= np.float32(factor)
    return tweak


def bias_moved(layer, by):
    def tweak(params):
        params[layer][1] += np.float32(by)
    return tweak


def zero_sum_taps(params):
    """The first layer's filters with taps that sum to zero per output channel AND per tap over the three colours, up to a small
    pattern t (zero-sum over the window): in the interior only the image term is left, at the borders the shift times the partial sums
    of t - as large as the image term, not a hundred times it."""
    w = params["c0"][0].astype(np.float64)
    t = np.random.default_rng(7).standard_normal((w.shape[0], 1) + w.shape[2:]) * 0.0008
    w = w - w.mean(axis=1, keepdims=True) + (t - t.mean(axis=(2, 3), keepdims=True))
    params["c0"][0][...] = w.astype(np.float16).astype(np.float32)


def element_type_cases():
    def up(y, B):      # every pooled value at the first pixel of its 2 x 2 window
        out = torch.zeros_like(y)
        out[:, :, ::2, ::2] = B["p"]
        return out
    return [HalfCase(*a, group="A", **kw) for a, kw in [
        # (the wrong evaluation shows only because `u` is scaled out of the half range: rounding an in-range float32 output moves it by
        #  2^-11 of itself, under TOL - what holds that path is the exact assertion of CONV_OUT_F32 and of the element size of `u`)
        (("convolution_element_types", C0 + conv("c1", "c0", 8) + conv("u", "c1", 8), "conv:c0 | conv:c1 | conv:u",
          Wrong("the float32 output rounded to halves", "u", patch={"u": lambda y, B: r16(y)})),
         dict(meta={"c0": PLAIN, "c1": PLAIN, "u": PLAIN}, f32=("data", "u"), flags={"c0": OUT16, "c1": F16, "u": F16 | OUT32}, tweak=scaled("u", 3e4))),
        (("convolution_sigmoid_second_top", C0 + conv("c1", "c0", 8) + sigmoid("sg", "c1", "sg"), "conv:c0 | conv:c1",
          Wrong("the second top without its Sigmoid", "sg", patch={"sg": lambda y, B: B["c1"]})),
         dict(meta={"c0": PLAIN, "c1": (False, "sg")}, f32=("data", "c1", "sg"), flags={"c0": OUT16, "c1": F16 | OUT32 | 2})),
        (("inner_product_element_types", C12 + fc("f1", "c0", 12) + relu("r1", "f1") + fc("f2", "f1", 8), "conv:c0 | inner_product:f1 | inner_product:f2",
          Wrong("the ReLU omitted", "f1", replace=(relu("r1", "f1"), ""))), dict(meta={"c0": PLAIN, "f1": FUSED, "f2": PLAIN}, f32=("data", "f2"))),
        (("depthwise_element_types", C0 + dwconv("d1", "c0", 8) + relu("r1", "d1") + dwconv("d2", "d1", 8), "conv:c0 | dwconv:d1 | dwconv:d2",
          Wrong("the ReLU omitted", "d1", replace=(relu("r1", "d1"), ""))), dict(meta={"c0": PLAIN, "d1": FUSED, "d2": PLAIN}, f32=("data", "d2"))),
        (("softmax_element_types", C12 + softmax("sm", "c0") + conv1("u", "sm", 12) + softmax("so", "u"), "conv:c0 | softmax:sm | conv:u | softmax:so",
          Wrong("the exponentials without their sum", "sm", patch={"sm": lambda y, B: torch.exp(B["c0"] - B["c0"].amax(dim=1, keepdim=True))})),
         dict(meta={"c0": PLAIN, "u": PLAIN}, f32=("data", "so"))),
        (("deconvolution_element_types", C12 + deconv("d1", "c0", 12) + conv1("u", "d1", 12) + deconv("d2", "u", 12), "conv:c0 | deconv:d1 | conv:u | deconv:d2",
          Wrong("the four phases of the stride written to one", "d1", patch={"d1": lambda y, B: y * (torch.arange(y.shape[2]).reshape(-1, 1) % 2 == 0)})),
         dict(meta={"c0": PLAIN, "u": PLAIN}, f32=("data", "d2"))),
        (("interp_element_types", C12 + interp("i1", "c0") + conv1("u", "i1", 12) + interp("i2", "u"), "conv:c0 | interp:i1 | conv:u | interp:i2",
          Wrong("the nearest pixel for the bilinear value", "i1", patch={"i1": lambda y, B: F.interpolate(B["c0"], size=tuple(y.shape[2:]), mode="nearest")})),
         dict(meta={"c0": PLAIN, "u": PLAIN}, f32=("data", "i2"))),
        (("upsample_element_types", C0 + pool("p", "c0", 2, 2, mask="pm") + upsample("u1", "p", "pm") + conv("u", "u1", 8) + pool("q", "u", 2, 2, mask="qm") +
          upsample("u2", "q", "qm"), "conv:c0 | maxpool:p | unpool:u1 | conv:u | maxpool:q | unpool:u2",
          Wrong("an Upsample that ignores the mask (the first pixel of every window)", "u1", patch={"u1": up})),
         dict(meta={"c0": PLAIN, "u": PLAIN}, f32=("data", "u2"), seed=2)),
    ]]


def image_cases():
    pw = power("pw", "data", "pw", "shift: %g" % SHIFT)
    net = pw + conv("c0", "pw", 8) + conv1("u", "c0", 4)
    meta = {"c0": PLAIN, "u": PLAIN}
    folded = dict(meta=meta, alias={"pw": ("data", 0)}, shift={"pw": SHIFT}, c=3, inputs="uniform")
    taken = dict(folded, f32=("u",), half_image=True, flags={"c0": F16 | ONES, "u": F16 | OUT32})
    upload = dict(folded, f32=("data", "pw", "u"), flags={"c0": OUT16, "u": F16 | OUT32})
    launched = dict(meta=meta, f32=("data", "pw", "u"), c=3, inputs="uniform", flags={"c0": OUT16, "u": F16 | OUT32})
    after = lambda y, B: r16(y + SHIFT) - SHIFT
    return [HalfCase(*a, group="B", **kw) for a, kw in [
        (("half_image", net, "conv:c0 | conv:u", Wrong("the shift added inside the zero padding", "c0", pad_value={"c0": SHIFT})), taken),
        (("half_image_5x5_stride_2", pw + conv("c0", "pw", 8, "kernel_size: 5 pad: 2 stride: 2") + conv1("u", "c0", 4), "conv:c0 | conv:u",
          Wrong("the shift applied twice on read-back", "pw", patch={"pw": lambda y, B: y + SHIFT})), taken),
        (("half_image_zero_sum_taps", net, "conv:c0 | conv:u", Wrong("the image rounded to halves after the shift", "c0", patch={"data": after})),
         dict(taken, tweak=zero_sum_taps)),
        (("half_image_switched_off", net, "conv:c0 | conv:u", Wrong("the shift not applied on read-back", "pw", patch={"pw": lambda y, B: y - SHIFT})),
         dict(upload, env={"FCN_F16_IMAGE": "0"})),
        (("half_image_without_fusion", net, "power:pw | conv:c0 | conv:u", Wrong("the Power launch left out", "pw", patch={"pw": lambda y, B: B["data"]})),
         dict(launched, engine=dict(fuse=False))),
        (("image_scale_2", power("pw", "data", "pw", "shift: -1 scale: 2") + conv("c0", "pw", 8) + conv1("u", "c0", 4), "power:pw | conv:c0 | conv:u",
          Wrong("the scale ignored", "pw", replace=(" scale: 2", ""))), launched),
        (("image_power_top_read_twice", net + conv("v", "pw", 8), "conv_group:c0+v | conv:u",
          Wrong("the second reader on the image without the shift", "v", replace=(conv("v", "pw", 8), conv("v", "data", 8)))),
         dict(upload, meta=dict(meta, v=PLAIN), f32=("data", "pw", "u", "v"), flags={"c0": OUT16, "v": 0, "u": F16 | OUT32})),
        (("image_power_top_is_an_output", pw + conv("c0", "data", 8) + conv1("u", "c0", 4), "power:pw | conv:c0 | conv:u",
          Wrong("the shift folded into an input that a convolution reads", "c0", patch={"data": lambda y, B: y + SHIFT})), launched),
        (("image_depthwise_first_layer", pw + dwconv("d", "pw", 3), "dwconv:d", Wrong("the shift added inside the zero padding", "d", pad_value={"d": SHIFT})),
         dict(folded, meta={"d": PLAIN}, f32=("data", "pw", "d"))),
        (("image_four_channels", net, "conv:c0 | conv:u", Wrong("the shift added inside the zero padding", "c0", pad_value={"c0": SHIFT})), dict(upload, c=4)),
    ]]


def view_cases():
    a, b, d = conv("a", "c0", 8), conv("b", "c0", 8), conv("d", "c0", 8)
    c16 = conv("c0", "data", 16)
    u = conv1("u", "cat", 8)
    swap = lambda x, y: Wrong("two Concat members swapped", "cat", replace=(bottoms([x, y]), bottoms([y, x])))
    tops = Wrong("the two Slice tops swapped", "v0", replace=('top: "s0" top: "s1"', 'top: "s1" top: "s0"'))
    runs = lambda y, B: torch.cat([y[:, :4], y[:, 8:12], y[:, 4:8], y[:, 12:]], 1)
    return [HalfCase(*a_, group="C", **kw) for a_, kw in [
        (("concat_view", C0 + a + b + concat("cat", ["a", "b"]) + u, "conv:c0 | conv_group:a+b | conv:u", swap("a", "b")),
         dict(meta={n: PLAIN for n in ("c0", "a", "b", "u")}, alias={"a": ("cat", 0), "b": ("cat", 8)}, f32=("data", "u"))),
        (("concat_copy_4_and_12_channels", C0 + conv("a", "c0", 4) + conv("b", "c0", 12) + concat("cat", ["a", "b"]) + u,
          "conv:c0 | conv_group:a+b | copy:cat:a | copy:cat:b | conv:u", Wrong("two 4-channel runs of the second member swapped", "cat", patch={"cat": runs})),
         dict(meta={n: PLAIN for n in ("c0", "a", "b", "u")}, copy_concats=("cat",), f32=("data", "u"))),
        (("concat_pooling_member_with_a_relu", C0 + a + pool("pl", "c0", 3, 1, 1) + relu("rp", "pl") + concat("cat", ["a", "pl"]) + u,
          "conv:c0 | conv:a {+pl} | relu:rp | conv:u", Wrong("the pooling's ReLU over its neighbour", "cat", patch={"cat": lambda y, B: y.clamp(min=0)})),
         dict(meta={n: PLAIN for n in ("c0", "a", "u")}, alias={"a": ("cat", 0), "pl": ("cat", 8)}, f32=("data", "u"), tweak=bias_moved("c0", -2.0))),
        (("concat_dropout_member", C0 + a + d + dropout("dr", "d") + concat("cat", ["a", "d"]) + u, "conv:c0 | conv_group:a+d | conv:u", swap("a", "d")),
         dict(meta={n: PLAIN for n in ("c0", "a", "d", "u")}, alias={"a": ("cat", 0), "d": ("cat", 8)}, f32=("data", "u"))),
        (("slice_views_at_8", c16 + slices("sl", "c0", ["s0", "s1"], 8) + conv1("v0", "s0", 8) + conv1("v1", "s1", 8), "conv:c0 | conv_group:v0+v1", tops),
         dict(meta={n: PLAIN for n in ("c0", "v0", "v1")}, alias={"s0": ("c0", 0), "s1": ("c0", 8)}, f32=("data", "v0", "v1"))),
        (("slice_copies_at_4", c16 + slices("sl", "c0", ["s0", "s1"], 4) + conv1("v0", "s0", 8) + conv1("v1", "s1", 8),
          "conv:c0 | copy:sl:s0 | copy:sl:s1 | conv_group:v0+v1", Wrong("the second copy from channel 0", "s1", patch={"s1": lambda y, B: B["c0"][:, :12]})),
         dict(meta={n: PLAIN for n in ("c0", "v0", "v1")}, copy_slices=("sl",), f32=("data", "v0", "v1"))),
        (("slice_of_a_concat_view", C0 + a + b + concat("cat", ["a", "b"]) + slices("sl", "cat", ["s0", "s1"], 8) + conv1("v0", "s0", 8) + conv1("v1", "s1", 8),
          "conv:c0 | conv_group:a+b | conv_group:v0+v1", tops),
         dict(meta={n: PLAIN for n in ("c0", "a", "b", "v0", "v1")}, alias={"a": ("cat", 0), "b": ("cat", 8), "s0": ("cat", 0), "s1": ("cat", 8)},
              f32=("data", "v0", "v1"))),
        (("dropout_to_another_top", C0 + dropout("dr", "c0", "d") + conv("v", "d", 8), "conv:c0 | conv:v",
          Wrong("a top of its own that nothing writes", "d", patch={"d": zero})), dict(meta={"c0": PLAIN, "v": PLAIN}, alias={"d": ("c0", 0)}, f32=("data", "v"))),
        (("crop_of_halves", C0 + pool("q", "c0", 2, 2) + crop("cr", "c0", "q") + conv1("u", "cr", 8), "conv:c0 | crop:cr | maxpool:q | conv:u",
          Wrong("the offset ignored", "cr", replace=("offset: 2", "offset: 0"))), dict(meta={"c0": PLAIN, "u": PLAIN}, f32=("data", "u"))),
    ]]


def pool_lrn_cases():
    u = conv1("u", "n", 8)
    rides = C0 + conv("a", "c0", 8) + pool("pl", "c0", 3, 1, 1) + conv1("pp", "pl", 8)
    out = [
        (("pool_lrn", C0 + pool("p", "c0", 3, 2) + lrn("n", "p") + u, "conv:c0 | pool_lrn:p+n | conv:u", Wrong("the middle blob at its zero fill", "p", patch={"p": zero})),
         dict(meta={"c0": PLAIN, "u": PLAIN}, lazy=("p",), raw={"p": (0,)}, f32=("data", "u"))),
        (("lrn_pool", C0 + lrn("n", "c0") + pool("p", "n", 3, 2) + conv1("u", "p", 8), "conv:c0 | pool_lrn:n+p | conv:u",
          Wrong("the middle blob at its zero fill", "n", patch={"n": zero})), dict(meta={"c0": PLAIN, "u": PLAIN}, lazy=("n",), raw={"n": (0,)}, f32=("data", "u"))),
        (("pool_lrn_conv_below_its_size", conv("c0", "data", 64) + pool("p", "c0", 3, 2) + lrn("n", "p") + conv1("k", "n", 64) + relu("kr", "k") + conv1("u", "k", 8),
          "conv:c0 | pool_lrn:p+n | conv:k | conv:u", Wrong("the ReLU omitted", "k", replace=(relu("kr", "k"), ""))),
         dict(meta={"c0": PLAIN, "k": FUSED, "u": PLAIN}, lazy=("p",), raw={"p": (0,)}, f32=("data", "u"), seed=2)),
        (("pool_lrn_conv", conv("c0", "data", 64) + pool("p", "c0", 3, 2) + lrn("n", "p") + conv1("k", "n", 64) + relu("kr", "k") + conv1("u", "k", 8),
          "conv:c0 | pool_lrn_conv:p+n+k | conv:u", Wrong("the normalised blob at its zero fill", "n", patch={"n": zero})),
         dict(meta={"c0": PLAIN, "k": FUSED, "u": PLAIN}, lazy=("p", "n"), raw={"p": (0,)}, f32=("data", "u"), shape=(1, 8, 256, 256), ties=())),
        (("pool_lrn_second_consumer", C0 + pool("p", "c0", 3, 2) + lrn("n", "p") + u + conv1("v", "p", 8), "conv:c0 | maxpool:p | lrn:n | conv:v | conv:u",
          Wrong("the middle blob at its zero fill", "v", patch={"p": zero})), dict(meta={"c0": PLAIN, "u": PLAIN, "v": PLAIN}, f32=("data", "u", "v"))),
        (("masked_pool_lrn", C0 + pool("p", "c0", 3, 2, mask="p_mask") + lrn("n", "p") + u, "conv:c0 | maxpool:p | lrn:n | conv:u",
          Wrong("the mask never written", "p_mask", patch={"p_mask": zero})), dict(meta={"c0": PLAIN, "u": PLAIN}, f32=("data", "u"))),
        (("poolings_of_their_own", C0 + pool("p1", "c0", 3, 2) + pool("p2", "c0", 3, 2, kind="AVE") + gpool("p3", "c0") + gpool("p4", "c0", "MAX") +
          "".join(conv1("u%d" % i, "p%d" % i, 8) for i in (1, 2, 3, 4)), "conv:c0 | avepool:p2 | avepool:p3 | maxpool:p4 | maxpool:p1 | conv_group:u1+u2+u3+u4",
          Wrong("the maximum for the average", "p2", replace=(pool("p2", "c0", 3, 2, kind="AVE"), pool("p2", "c0", 3, 2)))),
         dict(meta={n: PLAIN for n in ("c0", "u1", "u2", "u3", "u4")}, f32=("data", "u1", "u2", "u3", "u4"))),
        (("pooling_rides_below_16384_pixels", rides, "conv:c0 | conv:a {+pl} | conv:pp", Wrong("the pooling left out of the launch", "pl", patch={"pl": zero})),
         dict(meta={"c0": PLAIN, "a": PLAIN, "pp": PLAIN}, f32=("data", "a", "pp"), seed=2)),
        (("pooling_launches_at_16384_pixels", rides, "conv:c0 | maxpool:pl | conv:a | conv:pp", Wrong("the pooling left out", "pl", patch={"pl": zero})),
         dict(meta={"c0": PLAIN, "a": PLAIN, "pp": PLAIN}, f32=("data", "a", "pp"), shape=(1, 8, 128, 128), ties=())),
    ]
    return [HalfCase(*a, group="D", **kw) for a, kw in out]


def batchnorm_eltwise_cases():
    u = conv("u", "c0", 8)
    in_place = bnorm("bn", "c0", "c0") + scale("sc", "c0", "c0")
    apart = bnorm("bn", "c0", "b") + scale("sc", "b", "s") + relu("r", "s", "r")
    three = C0 + conv("a", "c0", 8) + conv("b", "c0", 8) + conv("c", "c0", 8)
    names = ["a", "b", "c"]
    return [HalfCase(*a, group="E", **kw) for a, kw in [
        (("bn_scale_relu_in_place", C0 + in_place + relu("r", "c0") + u, "conv:c0 | bn_apply:bn+sc+r | conv:u",
          Wrong("batch statistics", "c0", bn_global={"bn": False})), dict(meta={"c0": PLAIN, "u": PLAIN}, raw={"c0": (1, 2)}, f32=("data", "u"))),
        (("bn_scale_relu_separate_tops", C0 + apart + conv("u", "r", 8), "conv:c0 | bn_apply:bn+sc+r | conv:u",
          Wrong("a middle blob at its zero fill", "b", patch={"b": zero})),
         dict(meta={"c0": PLAIN, "u": PLAIN}, lazy=("b", "s"), raw={"b": (0,), "s": (0,)}, f32=("data", "u"))),
        (("bn_chain_cut_by_a_second_consumer", C0 + apart + conv("v", "b", 8) + conv("u", "r", 8), "conv:c0 | bn_apply:bn | bn_apply:sc+r | conv:v | conv:u",
          Wrong("the BatchNorm top at its zero fill", "v", patch={"b": zero})),
         dict(meta={"c0": PLAIN, "u": PLAIN, "v": PLAIN}, lazy=("s",), raw={"s": (0,)}, f32=("data", "u", "v"))),
        (("eltwise_three_bottoms", three + elt("e", names, "operation: SUM coeff: 1 coeff: -0.5 coeff: 2") + elt("m", names, "operation: MAX") +
          elt("pr", names, "operation: PROD") + conv1("ue", "e", 8) + conv1("um", "m", 8) + conv1("up", "pr", 8),
          "conv:c0 | conv_group:a+b+c | eltwise:e | eltwise:e | eltwise:m | eltwise:m | eltwise:pr | eltwise:pr | conv_group:ue+um+up",
          Wrong("an Eltwise coefficient dropped", "e", replace=(" coeff: 1 coeff: -0.5 coeff: 2", " coeff: 1 coeff: 1 coeff: 2"))),
         dict(meta={n: PLAIN for n in ("c0", "a", "b", "c", "ue", "um", "up")}, f32=("data", "ue", "um", "up"))),
        (("reader_ahead_of_the_relu", C0 + conv("s", "c0", 8) + relu("r0", "c0") + u, "conv:c0 | conv:s | relu:r0 | conv:u",
          Wrong("the ReLU applied ahead of the early reader", "s", replace=(conv("s", "c0", 8) + relu("r0", "c0"), relu("r0", "c0") + conv("s", "c0", 8)))),
         dict(meta={"c0": PLAIN, "s": PLAIN, "u": PLAIN}, f32=("data", "s", "u"))),
        (("eltwise_with_a_relu_of_its_own", C0 + conv("a", "c0", 8) + conv("b", "c0", 8) + elt("e", ["a", "b"], "operation: SUM") + relu("r", "e") + conv1("u", "e", 8),
          "conv:c0 | conv_group:a+b | eltwise:e | relu:r | conv:u", Wrong("the ReLU omitted", "e", replace=(relu("r", "e"), ""))),
         dict(meta={n: PLAIN for n in ("c0", "a", "b", "u")}, f32=("data", "u"))),
    ]]


def level_cases():
    halves = lambda y, B: torch.cat([y[:, 8:], y[:, :8]], 1)
    c0 = C0 + relu("c0r", "c0")
    pa, pb = conv1("pa", "c0", 32) + relu("par", "pa"), conv("pb", "c0", 32) + relu("pbr", "pb")
    tail = c0 + pa + pb + concat("cat", ["pa", "pb"]) + conv1("h1", "cat", 4) + conv1("h2", "cat", 16) + sigmoid("sg", "h2", "sg")
    tailed = dict(meta={"c0": FUSED, "pa": FUSED, "pb": FUSED, "h1": PLAIN, "h2": (False, "sg")}, alias={"pa": ("cat", 0), "pb": ("cat", 32)},
                  f32=("data", "h1", "h2", "sg"))
    one = Wrong("a head's sum over one producer only", "h1", patch={"cat": lambda y, B: torch.cat([y[:, :32], 0 * y[:, 32:]], 1)})
    return [HalfCase(*a, group="F", **kw) for a, kw in [
        (("level_of_3x3_and_1x1", C0 + conv("a", "c0", 8) + relu("ar", "a") + conv1("b", "c0", 8) + relu("br", "b") + concat("cat", ["a", "b"]) + conv1("u", "cat", 8),
          "conv:c0 | conv_group:a+b | conv:u", Wrong("two Concat members swapped", "cat", replace=(bottoms(["a", "b"]), bottoms(["b", "a"])))),
         dict(meta={"c0": PLAIN, "a": FUSED, "b": FUSED, "u": PLAIN}, alias={"a": ("cat", 0), "b": ("cat", 8)}, f32=("data", "u"))),
        (("group_2_of_8_channel_groups", conv("c0", "data", 16) + conv("g", "c0", 16, "kernel_size: 3 pad: 1 group: 2") + conv1("u", "g", 8),
          "conv:c0 | conv_group:g+g | conv:u", Wrong("the two groups' outputs swapped", "g", patch={"g": halves})),
         dict(meta={"c0": PLAIN, "g": PLAIN, "u": PLAIN}, f32=("data", "u"))),
        (("heads_without_the_tail", tail, "conv:c0 | conv_group:pa+pb | conv_group:h1+h2", one), tailed),
        (("heads_with_FCN_CONV_TAIL", tail, "conv:c0 | conv_group:pa+pb | conv_group:h1+h2", one), dict(tailed, env={"FCN_CONV_TAIL": "1"})),
    ]]


CASES = element_type_cases() + image_cases() + view_cases() + pool_lrn_cases() + batchnorm_eltwise_cases() + level_cases()
IDS = [c.name for c in CASES]
assert len(set(IDS)) == len(IDS)


# ---------------------------------------------------------------------------------------------------------------------- the reference
def parse(text, phase="TEST"):
    msg = proto.parse_text(text)
    spec = NetSpec(msg, phase)
    spec.infer()
    return msg, spec


def blob_plan(spec, fuse=True, half_image=True):
    """storage.plan_blobs as Engine._plan_buffers calls it for dtype="f16": pure, no GPU."""
    outputs = [b for b in spec.output_blobs() if b in spec.blob_shapes and b not in spec.mask_blobs]
    return S.plan_blobs(spec, spec.blob_shapes, spec.data_tops(), outputs, True, fuse, half_image)


def rounding_hooks(spec, plan, raw, unfolded=()):
    """(store, operands) of forward_net for the half-float engine whose blobs `plan` lays out.

    store: a blob of 2-byte elements is rounded to the nearest half each time a layer writes it - but for the writes listed in `raw`,
    which a fused launch keeps in registers, and for the Power top of a half image, which is the image's buffer read through a shift.
    operands, the rule of storage.param_layout: the filters of a Convolution or InnerProduct are halves when its bottom holds halves (the
    segment's esize is the bottom's).  Everything else stays float32: biases, the filters of a depthwise Convolution (DEPTHWISE: always
    float32) and of a depthwise Deconvolution (PLAIN), BatchNorm and Scale blobs, and the first layer's filters when it reads a float32
    image.  The convolution behind a half image reads the un-shifted halves plus two channels of ones, and its filters carry, per tap, the
    shift times the sum of the ROUNDED filters over the colours as a half plus the half of the remainder (storage.pack) - but for the
    layers in `unfolded`, which read the shifted image as it is (a wrong evaluation states its padding in those terms)."""
    esize = plan.esize
    views = {t: (d, s) for d, (t, s) in plan.half_inputs.items()}
    writes = {}

    def store(name, y):
        i = writes[name] = writes.get(name, -1) + 1
        if esize.get(name, 4) == 2 and name not in views and i not in raw.get(name, ()):
            return r16(y)
        return y

    def operands(l, x, P, B):
        if l.type not in ("Convolution", "InnerProduct") or spec.is_depthwise(l) or esize[l.bottoms[0]] != 2:
            return x, P
        w = r16(P[0])
        if l.bottoms[0] in views and l.name not in unfolded:
            d, s = views[l.bottoms[0]]
            term = s * w.double().sum(dim=1, keepdim=True)
            hi = term.to(torch.float16).double()
            lo = (term - hi).to(torch.float16).double()
            ones = torch.ones_like(B[d][:, :1])
            x, w = torch.cat([B[d], ones, ones], 1), torch.cat([w, hi.to(w.dtype), lo.to(w.dtype)], 1)
        return x, [w] + list(P[1:])
    return store, operands


def case_inputs(case, spec, seed):
    params = random_params(spec, seed)
    if case.tweak is not None:
        case.tweak(params)
    rng = np.random.default_rng([seed, 1])      # (not the stream the parameters were drawn from)
    shape = spec.input_shapes["data"]
    x = rng.random(shape) if case.inputs == "uniform" else rng.standard_normal(shape)
    return params, {"data": x.astype(np.float32)}


def evaluate(case, spec, params, x, fused, dtype=torch.float64, wrong=None):
    """Every blob as the half-float engine holds it (numpy float64) and forward_net's own return value: the reference rounded for the
    plan with or without fusion; `wrong`: the case's wrong evaluation, by the same rules."""
    text = case.text
    kw = {}
    if wrong is not None:
        if wrong.replace is not None:
            assert text.count(wrong.replace[0]) == 1, wrong.replace[0]
            spec = parse(text.replace(*wrong.replace))[1]
        assert wrong.replace or wrong.patch or wrong.pad_value or wrong.bn_global
        kw = dict(patch=wrong.patch, pad_value=wrong.pad_value, bn_global=wrong.bn_global)
    plan = blob_plan(spec, fused, case.env.get("FCN_F16_IMAGE", "1") != "0")
    store, operands = rounding_hooks(spec, plan, case.raw if fused else {}, unfolded=tuple((wrong.pad_value or {}) if wrong is not None else ()))
    out = forward_net(spec, as_torch(params, dtype=dtype), x, dtype=dtype, store=store, operands=operands, **kw)
    blobs = numpy_blobs(out[0])
    for name in blobs:      # a blob that a fused launch skipped is written, rounded, by its own layer when somebody reads it
        if plan.esize.get(name, 4) == 2 and name not in {t for t, _s in plan.half_inputs.values()}:
            blobs[name] = blobs[name].astype(np.float16).astype(np.float64)
    if wrong is None or "data" not in (wrong.patch or {}):
        blobs["data"] = np.asarray(x["data"], np.float64)      # an input reads back as the host array it was uploaded from
    return blobs, out, plan


@functools.lru_cache(maxsize=None)
def reference(index):
    """Case `index`, computed once and shared by the tests: the parameters and the input the engine gets; every blob by the plan with
    fusion and by the plan without; what every layer read and the two largest values of every MAX pooling window (with fusion)."""
    case = CASES[index]
    msg, spec = parse(case.text)
    params, x = case_inputs(case, spec, case.seed)
    fused, out, plan = evaluate(case, spec, params, x, True)
    unfused, _, plan_unfused = evaluate(case, spec, params, x, False)
    return dict(msg=msg, spec=spec, params=params, x=x, blobs=fused, unfused=unfused, plan=plan, plan_unfused=plan_unfused,
                seen={k: v.numpy() for k, v in out[2].items()}, top2={k: v.numpy() for k, v in out[3].items()})


def primary(case, ref):
    return ref["blobs"] if case.engine.get("fuse", True) else ref["unfused"]


# ------------------------------------------------------------------------------------- without a GPU: the interpreter, and the cases can fail
def test_interpreter_hooks_by_hand():
    """store, operands and the new layer types of forward_net on a three-layer net, against numpy."""
    text = ('input: "data" input_shape { dim: 1 dim: 2 dim: 3 dim: 3 }\n' + conv("c", "data", 2, "kernel_size: 1") + relu("r", "c") +
            elt("e", ["c", "c", "c"], "operation: SUM coeff: 1 coeff: 0.5 coeff: -2") + gpool("g", "e"))
    _, spec = parse(text)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, 2, 3, 3))
    w, b = rng.standard_normal((2, 2, 1, 1)), rng.standard_normal(2)
    h = lambda a: np.asarray(a, np.float64).astype(np.float16).astype(np.float64)
    log = []

    def store(name, y):
        log.append(name)
        return r16(y) if name in ("c", "e") else y

    def operands(l, x_, P, B):
        return x_, [r16(P[0])] + list(P[1:])
    plain = numpy_blobs(forward_net(spec, as_torch({"c": [w, b]}), {"data": x})[0])
    got = numpy_blobs(forward_net(spec, as_torch({"c": [w, b]}), {"data": x}, store=store, operands=operands)[0])
    c = np.einsum("oi,nihw->nohw", w[:, :, 0, 0], x) + b[None, :, None, None]
    assert np.allclose(plain["c"], np.maximum(c, 0), rtol=1e-13, atol=1e-13) and np.allclose(plain["e"], -0.5 * plain["c"], rtol=1e-13, atol=1e-13)
    cr = np.maximum(h(np.einsum("oi,nihw->nohw", h(w[:, :, 0, 0]), x) + b[None, :, None, None]), 0)      # rounded filters, rounded store, then the ReLU's store
    assert np.array_equal(got["c"], cr) and not np.array_equal(got["c"], plain["c"])
    e = h(h(cr + 0.5 * cr) - 2 * cr)      # pairwise, the partial result stored in the top
    assert np.array_equal(got["e"], e)
    assert np.allclose(got["g"], e.mean(axis=(2, 3), keepdims=True), rtol=1e-13, atol=0) and got["g"].shape == (1, 2, 1, 1)
    assert log == ["data", "c", "c", "e", "e", "g"]


def test_interpreter_layer_types_of_the_half_matrix():
    """DepthwiseConvolution, Deconvolution, Crop, Upsample and MAX global pooling against their formulas; Interp is tests/torch_interp_ref's."""
    import ref64
    import ref_unpool64
    text = ('input: "data" input_shape { dim: 2 dim: 3 dim: 6 dim: 4 }\n' + dwconv("d", "data", 3) + deconv("t", "data", 3) + pool("p", "data", 2, 2, mask="pm") +
            upsample("up", "p", "pm", 6, 4) + crop("cr", "data", "p", 1) + gpool("g", "data", "MAX"))
    _, spec = parse(text)
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, 3, 6, 4))
    P = {"d": [rng.standard_normal((3, 1, 3, 3)), rng.standard_normal(3)], "t": [rng.standard_normal((3, 1, 4, 4)), rng.standard_normal(3)]}
    B = numpy_blobs(forward_net(spec, as_torch(P), {"data": x})[0])
    d = np.stack([ref64.conv2d(x[:, c:c + 1], P["d"][0][c:c + 1], P["d"][1][c:c + 1], 1, 1)[:, 0] for c in range(3)], 1)
    _y, idx = ref_unpool64.max_pool_argmax(x, 2, 2, 0)
    for name, want in (("d", d), ("t", ref64.deconv_depthwise(x, P["t"][0][:, 0], P["t"][1], 4, 2, 1)), ("pm", idx), ("up", ref_unpool64.unpool(_y, idx, 6, 4)),
                       ("cr", x[:, :, 1:4, 1:3]), ("g", x.max(axis=(2, 3), keepdims=True))):
        assert B[name].shape == want.shape and np.allclose(B[name], want, rtol=1e-12, atol=1e-12), name


def test_a_fused_pool_lrn_pair_rounds_as_the_two_launches_do():
    """Why `raw` changes nothing behind a Pool -> LRN or LRN -> Pool launch: the maximum of halves is a half, and rounding is monotonic,
    so the maximum of rounded values is the rounded maximum - the blob that stays in registers may be rounded or not."""
    for name in ("pool_lrn", "lrn_pool", "pool_lrn_conv_below_its_size"):
        index = IDS.index(name)
        case, ref = CASES[index], reference(index)
        assert case.raw and set(case.raw) <= set(case.lazy)
        for blob, want in ref["blobs"].items():
            assert np.array_equal(ref["unfused"][blob], want), (name, blob)


def test_a_blob_that_a_layer_reads_is_no_output():
    """Why "a lazy middle blob is a net output" is no case of the matrix (as in the float32 module), and why a float32 middle blob is
    none either but for the two sides of a Sigmoid and the Power top of an input."""
    for index, case in enumerate(CASES):
        ref = reference(index)
        spec = ref["spec"]
        read = {b for l in spec.layers for b in l.bottoms}
        assert not set(spec.output_blobs()) & read, case.name
        for name, es in ref["plan"].esize.items():
            if es == 4 and name in read and name not in spec.data_tops():
                kinds = {q.type for q in ref["plan"].producers[name]} | {q.type for q in ref["plan"].consumers[name]}
                assert kinds & {"Sigmoid", "Power"}, (case.name, name)


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_plan_of_the_blobs(index):
    """What the pure planner decides is what the case states: element sizes, views, copies, the half image."""
    case, ref = CASES[index], reference(index)
    plan = ref["plan"] if case.engine.get("fuse", True) else ref["plan_unfused"]
    assert {n for n, es in plan.esize.items() if es == 4} == set(case.f32) and set(plan.esize.values()) <= {2, 4}
    assert (plan.alias, plan.shift, plan.copy_concats, plan.copy_slices) == (case.alias, case.shift, set(case.copy_concats), set(case.copy_slices))
    assert plan.half_inputs == ({"data": ("pw", SHIFT)} if case.half_image else {})
    for top in plan.half_inputs.values():
        assert plan.views[top[0]].lazy_shift == SHIFT and plan.views["data"].lazy_shift == 0.0 and plan.views["data"].upload_shift == 0.0


def worst_wrong(case, ref):
    blobs = primary(case, ref)
    wrong = evaluate(case, ref["spec"], ref["params"], ref["x"], case.engine.get("fuse", True), wrong=case.wrong)[0]
    return rel_err(wrong[case.wrong.blob], blobs[case.wrong.blob])


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_reference_shows_the_case_can_fail(index):
    case, ref = CASES[index], reference(index)
    blobs, spec = primary(case, ref), ref["spec"]
    assert set(blobs) == set(spec.blob_shapes) == set(ref["unfused"])
    # the wrong evaluation is ten thresholds away, on a blob the GPU test compares
    err = worst_wrong(case, ref)
    assert err >= WRONG_AT_LEAST, (case.wrong.what, err)
    # the inputs: every ReLU reads a tenth of its elements on each side of zero, no MAX pooling window holds a tie (among the rounded values)
    for l in spec.layers:
        if l.type == "ReLU":
            negative = (ref["seen"][l.name] < 0).mean()
            assert 0.1 <= negative <= 0.9, (l.name, negative)
    for name, two in ref["top2"].items():
        if case.ties is None or name in case.ties:
            assert not (two[..., 0] == two[..., 1]).any(), name
        else:      # exempt (the large shapes): only where a tie cannot show - the pooling writes no mask
            assert [len(l.tops) for l in spec.layers if l.name == name] == [1], name


def propagated(spec, plan):
    """The blobs behind a COMPUTED half blob: a layer that writes them reads a blob of halves that a layer wrote (not the half image,
    which is the input rounded, nor its Power top), or a blob behind one.  Only there can a flipped half have travelled."""
    image = set(plan.half_inputs) | {t for t, _s in plan.half_inputs.values()}
    noisy = {n for n, es in plan.esize.items() if es == 2 and n not in image}
    out = set()
    for l in spec.layers:
        if any(b in noisy or b in out for b in l.bottoms if not (l.type == "Crop" and b == l.bottoms[-1])):
            out.update(t for t in l.tops if t not in spec.mask_blobs)
    return out


def elem_bound(name, behind):
    return 4 * MEASURED_ELEM if name in behind else 1.0


def f32_against_f64(index, seed):
    """(worst rel_err, worst elem_err ratio at ELEM_TOL on a blob that is not `propagated`, the same on one that is) of the float32
    interpreter against the float64 one, both with the rounding hooks, over the blobs the GPU test compares and both plans."""
    case = CASES[index]
    spec = reference(index)["spec"]
    params, x = case_inputs(case, spec, seed)
    worst = [0.0, 0.0, 0.0]
    for fused in (True, False):
        want, _, plan = evaluate(case, spec, params, x, fused)
        got = evaluate(case, spec, params, x, fused, dtype=torch.float32)[0]
        behind = propagated(spec, plan)
        for name in want:
            if name not in spec.mask_blobs:
                worst[0] = max(worst[0], rel_err(got[name], want[name]))
                worst[1 + (name in behind)] = max(worst[1 + (name in behind)], elem_err(got[name], want[name], ELEM_TOL)[0])
    return worst


@functools.lru_cache(maxsize=None)
def measurement():
    per_case = [[f32_against_f64(index, CASES[index].seed + 100 * k) for k in range(SEEDS)] for index in range(len(CASES))]
    return per_case


def test_threshold_is_the_measured_one():
    per_case = measurement()
    worst_rel, worst_first, worst_behind = (max(seed[k] for seeds in per_case for seed in seeds) for k in range(3))
    print("F16PLAN measured float32 against float64: rel_err %.3g, elem_err ratio at 2^-10 %.3g (first half blobs) %.3g (behind them)" % (
        worst_rel, worst_first, worst_behind))
    assert abs(worst_rel / MEASURED_F32 - 1) <= 0.1 and abs(worst_behind / MEASURED_ELEM - 1) <= 0.1 and worst_first <= 1.0
    assert TOL == 4 * MEASURED_F32 and TOL <= 5e-3
    assert TOL <= min(worst_wrong(case, reference(i)) for i, case in enumerate(CASES)) / 10


def test_elementwise_allowance_passes_one_flipped_half_and_fails_two():
    """conftest.elem_err(.., 2^-10): one half ulp of a value is at most 2^-10 of it, so a single flip always passes; two ulps are at
    least 2^-10 of the value, and fail wherever the value is above the blob's rms by more than its distance to the next power of two."""
    import ref64
    index = IDS.index("convolution_element_types")
    ref = reference(index)
    assert "c0" not in propagated(ref["spec"], ref["plan"]) and elem_bound("c0", propagated(ref["spec"], ref["plan"])) == 1.0
    b = ref["blobs"]["c0"]
    ulp = ref64.f16_ulp(b)
    for sign in (1.0, -1.0):
        assert elem_err(b + sign * ulp, b, ELEM_TOL)[0] <= 1.0
    rms = np.sqrt(np.mean(b * b))
    loud = 2 * ulp > ELEM_TOL * (np.abs(b) + rms)
    assert loud.mean() > 0.05
    flat = np.flatnonzero(loud.ravel())
    for i in flat[:: max(len(flat) // 16, 1)]:
        two = b.copy().ravel()
        two[i] += 2 * ulp.ravel()[i]
        assert elem_err(two, b.ravel(), ELEM_TOL)[0] > 1.0


# --------------------------------------------------------------------------------------------------- without a GPU: what storage refuses
SSD_HEAD = ('layer { name: "pm" type: "Permute" bottom: "c0" top: "pm" permute_param { order: 0 order: 2 order: 3 order: 1 } }\n'
            'layer { name: "fl" type: "Flatten" bottom: "pm" top: "fl" flatten_param { axis: 1 } }\n')
ROI = ('input: "rois" input_shape { dim: 3 dim: 5 }\n', 'layer { name: "rp" type: "ROIPooling" bottom: "c0" bottom: "rois" top: "rp" '
       'roi_pooling_param { pooled_h: 2 pooled_w: 2 spatial_scale: 1 } }\n')
STORAGE_REFUSALS = [
    ("ssd_head", "", C0 + SSD_HEAD, "layer type Permute (pm) has no half-float kernel"),
    ("region_layer", ROI[0], C0 + ROI[1], "layer type ROIPooling (rp) has no half-float kernel"),
    ("pooling_top_is_an_output", "", C0 + pool("p", "c0", 3, 2), "float32 blob p is produced by ['Pooling']"),
    ("view_of_a_root_with_another_element_size", "", C0 + conv("a", "c0", 8) + sigmoid("sg", "a", "sg") + dropout("dr", "a", "d") + conv("u", "d", 8),
     "blob d (2-byte elements) is a view of a (4-byte)"),
    ("deconvolution_with_group_1", "", C0 + deconv("t", "c0", 8, group=1) + conv1("u", "t", 8), "layer type Deconvolution with group 1 (t) has no half-float kernel"),
]


@pytest.mark.parametrize("name,head,body,message", STORAGE_REFUSALS, ids=[r[0] for r in STORAGE_REFUSALS])
def test_storage_refuses(name, head, body, message):
    _, spec = parse(head + 'input: "data" input_shape { dim: 2 dim: 8 dim: 11 dim: 10 }\n' + body)
    with pytest.raises(NotImplementedError) as e:
        plan = blob_plan(spec)
        S.param_layout(spec, plan.views, True)
    assert message in str(e.value) and str(e.value).startswith("f16 engine: ")


# ------------------------------------------------------------------------------------------------------------------- on the GPU
def make_engine(case, ref, **kw):
    from fcn_object_detector_amd.engine import Engine
    eng = Engine(NetSpec(ref["msg"], "TEST"), params={k: [a.copy() for a in v] for k, v in ref["params"].items()}, device=0, autotune=False, dtype="f16", **kw)
    eng.host_array("data")[...] = ref["x"]["data"]
    return eng


def compare(eng, want_blobs, names, worst, behind):
    for name in names:
        got, want = eng.read_blob(name), want_blobs[name]
        assert got.shape == want.shape, name
        worst[name] = max(worst.get(name, 0.0), rel_err(got, want))
        assert worst[name] < TOL, (name, worst[name])
        assert elem_err(got, want, ELEM_TOL)[0] <= elem_bound(name, behind), (name, elem_err(got, want, ELEM_TOL))


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_forward_plan_path_f16(gpu, monkeypatch, index):
    case, ref = CASES[index], reference(index)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    spec = ref["spec"]
    names = list(spec.blob_shapes)
    worst = {}
    eng = make_engine(case, ref, **case.engine)
    try:
        # 1. the path
        assert launch_list(eng) == case.launches
        assert eng._conv_layer_meta == {k: dict(relu=r, sigmoid_top=s) for k, (r, s) in case.meta.items()}
        assert (eng.alias, eng.shift) == (case.alias, case.shift)
        assert (eng.copy_concats, eng.copy_slices, set(eng._lazy_blob_ops)) == (set(case.copy_concats), set(case.copy_slices), set(case.lazy))
        assert {n: b.esize for n, b in eng.blobs.items()} == {n: 4 if n in case.f32 else 2 for n in names if n not in spec.mask_blobs}
        assert eng._half_inputs == ({"data": ("pw", SHIFT)} if case.half_image else {})
        flags = eng._conv_flags      # Convolution layer -> the flags of its descriptor
        assert set(flags) == {l.name for l in spec.layers if l.type == "Convolution"}
        assert {k: flags[k] & ~R for k in case.flags} == case.flags
        assert all(bool(f & ONES) == (case.half_image and n == "c0" and eng.blobs["data"].cstride == 8) for n, f in flags.items())
        for top, sh in case.shift.items():      # the half image is uploaded as it is and its Power top read through the shift; a float32 image is uploaded shifted
            root = eng.blobs[eng.alias[top][0]]
            assert (root.upload_shift, root.lazy_shift, eng.blobs[top].lazy_shift) == ((0.0, 0.0, sh) if case.half_image else (sh, -sh, 0.0))
        # 2. and 3.: the lazy blobs ahead of the others, a forward behind them, the lazy blobs behind the others, a forward without a graph
        want = primary(case, ref)
        behind = {fuse: propagated(spec, ref["plan" if fuse else "plan_unfused"]) for fuse in (True, False)}
        mine = behind[case.engine.get("fuse", True)]
        plain = [n for n in names if n not in case.lazy]
        first = copies(eng.forward())
        assert set(first) == set(spec.output_blobs()) - set(spec.mask_blobs)
        compare(eng, want, list(case.lazy) + plain, worst, mine)
        again = copies(eng.forward())
        assert same_bits(first, again)
        compare(eng, want, plain + list(case.lazy), worst, mine)
        assert same_bits(first, copies(eng.forward()))
        assert same_bits(first, copies(eng.forward(use_graph=False)))
    finally:
        eng.close()
    for kw, want in ((dict(fuse=False, group_convs=False), ref["unfused"]), (dict(fuse=True, group_convs=False), ref["blobs"])):
        eng = make_engine(case, ref, **kw)
        try:
            eng.forward()
            compare(eng, want, names, worst, behind[kw["fuse"]])
        finally:
            eng.close()
    print("PLANPATH16 %s %s %s" % (case.group, IDS[index], " ".join("%s %.2g" % kv for kv in worst.items())))


INPUT8 = 'input: "data" input_shape { dim: 2 dim: 8 dim: 11 dim: 10 }\n'
LABEL = 'input: "label" input_shape { dim: 2 dim: 1 dim: 11 dim: 10 }\n'
ENGINE_REFUSALS = [
    ("train_phase", INPUT8 + C0, dict(phase="TRAIN"), "the half-float path is inference only"),
    ("dilated_convolution", INPUT8 + C0 + conv("k", "c0", 8, "kernel_size: 3 pad: 2 dilation: 2"), {}, "f16 engine: Convolution k with dilation 2 has no half-float kernel"),
    ("rectangular_convolution", INPUT8 + C0 + conv("k", "c0", 8, "kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 1"), {},
     "f16 engine: rectangular Convolution k (1x3 stride 1x1 pad 0x1) has no half-float kernel"),
    ("accuracy", INPUT8 + LABEL + C0 + 'layer { name: "acc" type: "Accuracy" bottom: "c0" bottom: "label" top: "acc" }\n', {},
     "f16 engine: layer type Accuracy (acc) has no half-float kernel"),
    ("leaky_relu_over_halves", INPUT8 + C0 + relu("r", "c0", slope=0.1) + conv("u", "c0", 8), {}, "f16 engine: ReLU r with a negative slope"),
    ("lrn_local_size_3", INPUT8 + C0 + pool("p", "c0", 3, 2) + lrn("n", "p", 3) + conv1("u", "n", 8), {},
     "f16 engine: LRN n with local_size 3 (the half-float kernel takes 5 only)"),
    ("max_pooling_of_12_half_channels", INPUT8 + C12 + pool("p", "c0", 3, 2) + conv1("u", "p", 8), {},
     "f16 engine: MAX pooling p over 12 channels (the half-float kernels take whole 8-channel segments)"),
    ("lrn_of_12_half_channels", INPUT8 + C12 + lrn("n", "c0") + conv1("u", "n", 8), {},
     "f16 engine: LRN n over 12 channels (the half-float kernel takes whole 8-channel segments)"),
    ("batchnorm_with_batch_statistics", INPUT8 + C0 + unary("BatchNorm", "bn", "c0", "c0", " batch_norm_param { use_global_stats: false }") + conv("u", "c0", 8), {},
     "f16 engine: BatchNorm bn with batch statistics"),
    ("eltwise_of_half_and_float32", INPUT8 + C0 + conv("a", "c0", 8) + sigmoid("sg", "a", "sg") + elt("e", ["a", "c0"], "operation: SUM") + conv1("u", "e", 8), {},
     "f16 engine: Eltwise e mixes half and float32 blobs"),
    ("concat_copy_of_half_and_float32", INPUT8 + C0 + concat("cat", ["data", "c0"]) + conv1("u", "cat", 8), {}, "f16 engine: cat:data copies between half and float32 blobs"),
    ("crop_of_float32_into_halves", INPUT8 + C0 + pool("q", "c0", 2, 2) + crop("cr", "data", "q") + conv1("u", "cr", 8), {},
     "f16 engine: Crop cr copies between half and float32 blobs"),
    ("batchnorm_chain_of_float32_into_halves", INPUT8 + scale("sc", "data", "s") + conv("u", "s", 8), {}, "f16 engine: Scale sc between half and float32 blobs"),
    ("inner_product_of_float32_into_halves", INPUT8 + fc("f1", "data", 8) + fc("f2", "f1", 8), {}, "f16 engine: InnerProduct f1 reads float32 and writes halves"),
    ("interp_of_float32_into_halves", INPUT8 + interp("i", "data") + conv("u", "i", 8), {}, "f16 engine: Interp i reads the float32 blob data and writes halves"),
    ("upsample_of_float32_into_halves", INPUT8 + C0 + pool("p", "c0", 2, 2, mask="pm") + conv("a", "p", 8) + sigmoid("sg", "a", "sg") + upsample("up", "a", "pm") +
     conv("u", "up", 8), {}, "f16 engine: Upsample up reads the float32 blob a and writes halves"),
    ("grouped_convolution_splits_a_segment", 'input: "data" input_shape { dim: 2 dim: 16 dim: 11 dim: 10 }\n' + conv("g", "data", 8, "kernel_size: 3 pad: 1 group: 2") +
     conv("u", "g", 8), {}, "grouped Convolution g: a fused Sigmoid, a folded input shift or output groups of 4 channels"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,text,kw,message", ENGINE_REFUSALS, ids=[r[0] for r in ENGINE_REFUSALS])
def test_engine_refuses(gpu, name, text, kw, message):
    from fcn_object_detector_amd.engine import Engine
    msg = proto.parse_text(text)
    spec = NetSpec(msg, kw.get("phase", "TEST"))
    spec.infer()
    with pytest.raises(NotImplementedError) as e:
        Engine(spec, params=random_params(spec, 1), device=0, autotune=False, dtype="f16").close()
    assert message in str(e.value)
