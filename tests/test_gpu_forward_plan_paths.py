"""The forward planner's fusion, view and level paths, one tiny net per path, every blob against float64.

Every case is a prototxt of a few layers over `data` (2 x C x 11 x 10, C = 4 or 8), run as Engine(NetSpec(msg, phase), params=...,
device=0, autotune=False) with seeded parameters (torch_resnet_ref.random_params) and default_rng inputs.  A case states, and the GPU test
asserts, (1) the plan: the whole launch list of eng.ops as (kind, label) pairs - the label without its "[cfg.. ..wg]" part, with its
"{+pool}" and "{tail: ...}" parts - and eng.alias, eng.copy_concats, eng.copy_slices, eng.shift, eng._conv_layer_meta and the keys of
eng._lazy_blob_ops, all of them exactly; (2) every blob of the net through eng.read_blob against tests/torch_forward_ref.forward_net, the
lazy blobs once before and once behind the others; (3) identical bits of all outputs from forward() twice, from a forward() behind the
lazy reads and from forward(use_graph=False).  (2) is repeated with fuse=False, group_convs=False and with fuse=True, group_convs=False.

The matrix (K: Convolution and InnerProduct both):
  A  epilogues      K + in-place ReLU (fused); + leaky ReLU (own launch); + ReLU to another top (not fused, the top keeps pre-ReLU values);
                    a reader of the top listed BEFORE the in-place ReLU (not fused; the reader runs ahead of the ReLU launch and sees pre-ReLU
                    values, a later reader sees post-ReLU ones).  Convolution -> Sigmoid to a second top, one consumer (one launch writes
                    both); refused for a Sigmoid in place, a second reader of the convolution top, an in-place layer between the two.
                    (An InnerProduct never carries a Sigmoid: the planner has no such path.)
  B  levels         a tiny inception module with a group: 2 branch (the pooling rides in the first launch, the Concat is a view); three
                    fusable MAX poolings beside two convolutions (two ride, one launches); 9 convolutions and a pooling (it does not ride);
                    17 convolutions (two launches); a level of poolings alone ahead of a level whose launch takes one (no leak).
  C  pool / LRN     Pool -> LRN, LRN -> Pool, Pool(3, 2) -> LRN(5) -> 1x1 Convolution 64 -> 64 + ReLU as single launches whose middle blobs
                    are lazy; the two-launch plan for a second consumer of the middle blob, local_size 3, AVE pooling, a mask top.
  D  views          Concat as views (Convolution, Pooling + in-place ReLU, in-place Dropout; the pooling in the middle and in front);
                    Concat that copies (second reader, 6 channels, a bottom twice, a net input, a Concat top); Slice as views (offsets 0
                    and 8; Convolution, Pooling and Concat read them) and as copies (slice point 5; Eltwise readers); a Slice of a Concat
                    view; Dropout to another top as an alias; Power shift -0.5 folded into the upload ahead of a PADDED convolution, and
                    launched for scale 2 or an input with a second reader.
  E  BatchNorm      BatchNorm -> Scale -> ReLU in place and with separate tops (lazy middles), cut by a second consumer, Scale -> ReLU
                    alone, ended by a leaky ReLU - each with TEST global statistics and with TRAIN batch statistics.
  F  tail           FCN_CONV_TAIL=1: a 64-channel blob of two 32-output ReLU convolutions on one level and on two; 1, 2 and 4 heads, one
                    with a Sigmoid second top; refused for a 16-channel producer, a 3-output head, a pooling that writes part, a 3x3 head.
Two cases of the issue cannot be built: "the middle blob is a net output" (C) and "a middle top is an output" (E).  A net output is a top
no layer reads (NetSpec.output_blobs), and the middle blob of a pair or chain is read by its second layer; the CPU part holds that rule.

The part without a GPU shows on the reference alone that each case CAN fail: Case.wrong names the wrong evaluation the case guards against
(ReLU applied to the early reader, a middle blob left at its zero fill, two Concat members swapped, the shift added to the padding, batch
statistics for global ones, a head's sum over one producer only, ...), computed by the interpreter from a mutated prototxt or with a
patched blob.  It must differ from the right value by at least 100 x 1e-4 in rel_err on a blob the GPU test compares, while the float32
evaluation of the same net stays under 1e-5 of the float64 one: the threshold sits a hundredfold under any of those mistakes and tenfold
over float32 rounding.  The inputs are held to what that needs: a tenth of the elements every ReLU reads on each side of zero, no MAX
pooling window with a tie.

Thresholds: tests/test_gpu_backward_fanout.py's blob threshold, rel_err < 1e-4, and conftest.elem_err(.., 1e-4) <= 1."""
import functools
import re
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import pytest
import torch

from conftest import elem_err, rel_err
from fcn_object_detector_amd import proto
from fcn_object_detector_amd.netspec import NetSpec
from torch_forward_ref import forward_net
from torch_resnet_ref import as_torch, random_params

TOL, WRONG_AT_LEAST, F32_AT_MOST = 1e-4, 100 * 1e-4, 1e-5
FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'


# ------------------------------------------------------------------------------------------------------------------ prototxt snippets
def conv(name, bottom, n, geometry="kernel_size: 3 pad: 1"):
    return 'layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: %d %s %s } }\n' % (
        name, bottom, name, n, geometry, FILL)


def conv1(name, bottom, n):
    return conv(name, bottom, n, "kernel_size: 1")


def fc(name, bottom, n):
    return 'layer { name: "%s" type: "InnerProduct" bottom: "%s" top: "%s" inner_product_param { num_output: %d %s } }\n' % (name, bottom, name, n, FILL)


def unary(kind, name, bottom, top=None, param=""):
    return 'layer { name: "%s" type: "%s" bottom: "%s" top: "%s"%s }\n' % (name, kind, bottom, top or bottom, param)


def relu(name, bottom, top=None, slope=None):
    return unary("ReLU", name, bottom, top, "" if slope is None else " relu_param { negative_slope: %g }" % slope)


def sigmoid(name, bottom, top=None):
    return unary("Sigmoid", name, bottom, top)


def dropout(name, bottom, top=None):
    return unary("Dropout", name, bottom, top, " dropout_param { dropout_ratio: 0.4 }")


def power(name, bottom, top, param):
    return unary("Power", name, bottom, top, " power_param { %s }" % param)


def pool(name, bottom, k, s, pad=0, kind="MAX", mask=None):
    return 'layer { name: "%s" type: "Pooling" bottom: "%s" top: "%s"%s pooling_param { pool: %s kernel_size: %d stride: %d pad: %d } }\n' % (
        name, bottom, name, ' top: "%s"' % mask if mask else "", kind, k, s, pad)


def lrn(name, bottom, size=5):
    return unary("LRN", name, bottom, name, " lrn_param { local_size: %d alpha: 0.5 beta: 0.75 }" % size)


def bottoms(names):
    return " ".join('bottom: "%s"' % b for b in names)


def concat(name, names):
    return 'layer { name: "%s" type: "Concat" %s top: "%s" }\n' % (name, bottoms(names), name)


def slices(name, bottom, tops, point):
    return 'layer { name: "%s" type: "Slice" bottom: "%s" %s slice_param { slice_point: %d } }\n' % (name, bottom, " ".join('top: "%s"' % t for t in tops), point)


def elt(name, names, param):
    return 'layer { name: "%s" type: "Eltwise" %s top: "%s" eltwise_param { %s } }\n' % (name, bottoms(names), name, param)


def bnorm(name, bottom, top):
    return unary("BatchNorm", name, bottom, top)


def scale(name, bottom, top):
    return unary("Scale", name, bottom, top, " scale_param { bias_term: true }")


# ----------------------------------------------------------------------------------------------------------------------- the table
def zero(y, B):
    return torch.zeros_like(y)


@dataclass(frozen=True)
class Wrong:
    """A wrong evaluation of the case's net and the blob on which it shows: `replace` (old, new) mutates the prototxt, the rest are the
    hooks of forward_net."""
    what: str
    blob: str
    replace: Optional[Tuple[str, str]] = None
    patch: Optional[Dict[str, Callable]] = None
    pad_value: Optional[Dict[str, float]] = None
    bn_global: Optional[Dict[str, bool]] = None


@dataclass(frozen=True)
class Case:
    """One path.  body: the layers behind the input; ops: the launch list "kind:label | kind:label | ..."; meta: layer -> (ReLU in the
    epilogue, the top of a Sigmoid in it) for every Convolution and InnerProduct; alias / shift / copy_concats / copy_slices / lazy: the
    storage plan, complete; c: channels of `data`; inputs: "normal", "normal-1.45" (most MAX windows of 3 x 3 straddle zero) or
    "uniform" ([0, 1): the image a Power shift centres); tail: FCN_CONV_TAIL=1; seed: of the parameters and the input (another one where the
    first fails the conditions the part without a GPU holds the inputs to)."""
    name: str
    body: str
    ops: str
    wrong: Wrong
    meta: Dict[str, tuple] = field(default_factory=dict)
    alias: Dict[str, tuple] = field(default_factory=dict)
    shift: Dict[str, float] = field(default_factory=dict)
    copy_concats: tuple = ()
    copy_slices: tuple = ()
    lazy: tuple = ()
    c: int = 4
    phase: str = "TEST"
    inputs: str = "normal"
    tail: bool = False
    seed: int = 1

    @property
    def text(self):
        return 'input: "data" input_shape { dim: 2 dim: %d dim: 11 dim: 10 }\n' % self.c + self.body

    @property
    def launches(self):
        return [tuple(o.split(":", 1)) for o in self.ops.split(" | ")]


PLAIN, FUSED = (False, None), (True, None)


def epilogue_cases():
    out = []
    for k, lay, op in (("convolution", lambda n, b: conv(n, b, 8), "conv"), ("inner_product", lambda n, b: fc(n, b, 8), "inner_product")):
        c0, u, s = lay("c0", "data"), lay("u", "c0"), lay("s", "c0")
        o = lambda text: text.replace("K:", op + ":")
        out += [
            Case(k + "_relu_fused", c0 + relu("r0", "c0") + u, o("K:c0 | K:u"), Wrong("the ReLU omitted", "c0", replace=(relu("r0", "c0"), "")),
                 meta={"c0": FUSED, "u": PLAIN}),
            Case(k + "_relu_leaky", c0 + relu("r0", "c0", slope=0.1) + u, o("K:c0 | relu:r0 | K:u"),
                 Wrong("the slope dropped", "c0", replace=(" relu_param { negative_slope: 0.1 }", "")), meta={"c0": PLAIN, "u": PLAIN}),
            Case(k + "_relu_to_another_top", c0 + relu("r0", "c0", "r") + lay("u", "r"), o("K:c0 | relu:r0 | K:u"),
                 Wrong("the ReLU written over the layer's own top", "c0", patch={"c0": lambda y, B: y.clamp(min=0)}), meta={"c0": PLAIN, "u": PLAIN}),
            Case(k + "_reader_ahead_of_the_relu", c0 + s + relu("r0", "c0") + u, o("K:c0 | K:s | relu:r0 | K:u"),
                 Wrong("the ReLU applied ahead of the early reader", "s", replace=(s + relu("r0", "c0"), relu("r0", "c0") + s)),
                 meta={"c0": PLAIN, "s": PLAIN, "u": PLAIN}),
        ]
    c0 = conv("c0", "data", 8)
    out += [
        Case("sigmoid_second_top", c0 + sigmoid("sg", "c0", "sg"), "conv:c0", Wrong("the second top without its Sigmoid", "sg", patch={"sg": lambda y, B: B["c0"]}),
             meta={"c0": (False, "sg")}),
        Case("sigmoid_in_place", c0 + sigmoid("sg", "c0") + conv("u", "c0", 8), "conv:c0 | sigmoid:sg | conv:u",
             Wrong("the Sigmoid omitted", "c0", replace=(sigmoid("sg", "c0"), "")), meta={"c0": PLAIN, "u": PLAIN}),
        Case("sigmoid_top_with_a_second_reader", c0 + sigmoid("sg", "c0", "sg") + conv("u", "c0", 8), "conv:c0 | sigmoid:sg | conv:u",
             Wrong("the Sigmoid written over the convolution top", "u", patch={"c0": lambda y, B: torch.sigmoid(y)}), meta={"c0": PLAIN, "u": PLAIN}),
        Case("sigmoid_behind_an_in_place_layer", c0 + relu("r0", "c0", slope=0.1) + sigmoid("sg", "c0", "sg"), "conv:c0 | relu:r0 | sigmoid:sg",
             Wrong("the Sigmoid of the convolution's own output", "sg", replace=(relu("r0", "c0", slope=0.1), "")), meta={"c0": PLAIN}),
    ]
    return out


def _many(n):
    names = ["k%d" % i for i in range(1, n + 1)]
    return "".join(conv1(k, "data", 4) for k in names), names


def level_cases():
    inception = (conv1("b1", "data", 8) + relu("b1r", "b1") + conv1("b3r", "data", 8) + relu("b3rr", "b3r") + conv("b3", "b3r", 8, "kernel_size: 3 pad: 1 group: 2") +
                 relu("b3_r", "b3") + conv1("b5r", "data", 8) + relu("b5rr", "b5r") + conv("b5", "b5r", 8, "kernel_size: 5 pad: 2") + relu("b5_r", "b5") +
                 pool("pl", "data", 3, 1, 1) + conv1("pp", "pl", 8) + relu("pp_r", "pp"))
    k9, n9 = _many(9)
    k17, n17 = _many(17)
    return [
        Case("inception_module", inception + concat("cat", ["b1", "b3", "b5", "pp"]), "conv_group:b1+b3r+b5r {+pl} | conv_group:b3+b3+b5+pp",
             Wrong("two Concat members swapped", "cat", replace=(bottoms(["b1", "b3"]), bottoms(["b3", "b1"]))), c=8,
             meta={n: FUSED for n in ("b1", "b3r", "b3", "b5r", "b5", "pp")}, alias={"b1": ("cat", 0), "b3": ("cat", 8), "b5": ("cat", 16), "pp": ("cat", 24)}),
        Case("three_poolings_two_convolutions", pool("p1", "data", 3, 1, 1) + pool("p2", "data", 2, 2) + pool("p3", "data", 3, 2) + conv("c1", "data", 8) +
             conv1("c2", "data", 8), "conv_group:c1+c2 {+p1+p2} | maxpool:p3", Wrong("the third pooling skipped", "p3", patch={"p3": zero}), c=8,
             meta={"c1": PLAIN, "c2": PLAIN}),
        Case("nine_convolutions_one_pooling", k9 + pool("p", "data", 3, 2) + concat("cat", n9), "conv_group:%s | maxpool:p" % "+".join(n9),
             Wrong("the ninth convolution left out", "cat", patch={"k9": zero}), c=8, meta={n: PLAIN for n in n9},
             alias={n: ("cat", 4 * i) for i, n in enumerate(n9)}),
        Case("seventeen_convolutions", k17 + concat("cat", n17), "conv_group:%s | conv:k17" % "+".join(n17[:16]),
             Wrong("the seventeenth convolution left out", "cat", patch={"k17": zero}), c=8, meta={n: PLAIN for n in n17},
             alias={n: ("cat", 4 * i) for i, n in enumerate(n17)}),
        Case("pooling_alone_on_a_level", pool("p0", "data", 3, 1, 1) + pool("a", "data", 3, 1, 1, "AVE") + conv("c1", "p0", 8) + pool("q", "a", 3, 2),
             "avepool:a | maxpool:p0 | conv:c1 {+q}",
             Wrong("the convolution run beside the pooling it reads (on the zero fill)", "c1", patch={"p0": zero}), c=8, meta={"c1": PLAIN}),
    ]


def pool_lrn_cases():
    c0 = conv("c0", "data", 8)
    c64 = conv("c0", "data", 64)
    u = conv1("u", "n", 4)
    return [
        Case("pool_lrn", c0 + pool("p", "c0", 3, 2) + lrn("n", "p") + u, "conv:c0 | pool_lrn:p+n | conv:u", Wrong("the middle blob at its zero fill", "p", patch={"p": zero}),
             meta={"c0": PLAIN, "u": PLAIN}, lazy=("p",)),
        Case("lrn_pool", c0 + lrn("n", "c0") + pool("p", "n", 3, 2) + conv1("u", "p", 4), "conv:c0 | pool_lrn:n+p | conv:u",
             Wrong("the middle blob at its zero fill", "n", patch={"n": zero}), meta={"c0": PLAIN, "u": PLAIN}, lazy=("n",)),
        Case("pool_lrn_conv", c64 + pool("p", "c0", 3, 2) + lrn("n", "p") + conv1("k", "n", 64) + relu("kr", "k"), "conv:c0 | pool_lrn_conv:p+n+k",
             Wrong("the normalised blob at its zero fill", "n", patch={"n": zero}), meta={"c0": PLAIN, "k": FUSED}, lazy=("p", "n")),
        Case("pool_lrn_second_consumer", c0 + pool("p", "c0", 3, 2) + lrn("n", "p") + u + conv1("v", "p", 4), "conv:c0 | maxpool:p | lrn:n | conv:v | conv:u",
             Wrong("the middle blob at its zero fill", "v", patch={"p": zero}), meta={"c0": PLAIN, "u": PLAIN, "v": PLAIN}),
        Case("pool_lrn_local_size_3", c0 + pool("p", "c0", 3, 2) + lrn("n", "p", 3) + u, "conv:c0 | maxpool:p | lrn:n | conv:u",
             Wrong("the single pass's five channels", "n", replace=("local_size: 3", "local_size: 5")), meta={"c0": PLAIN, "u": PLAIN}),
        Case("ave_pool_lrn", c0 + pool("p", "c0", 3, 2, kind="AVE") + lrn("n", "p") + u, "conv:c0 | avepool:p | lrn:n | conv:u",
             Wrong("the single pass's maximum", "p", replace=("pool: AVE", "pool: MAX")), meta={"c0": PLAIN, "u": PLAIN}),
        Case("masked_pool_lrn", c0 + pool("p", "c0", 3, 2, mask="p_mask") + lrn("n", "p") + u, "conv:c0 | maxpool:p | lrn:n | conv:u",
             Wrong("the mask never written", "p_mask", patch={"p_mask": zero}), meta={"c0": PLAIN, "u": PLAIN}),
    ]


def view_cases():
    a, b, c = conv("a", "data", 8), conv("b", "data", 8), conv("c", "data", 8)
    members = a + pool("pl", "data", 3, 1, 1) + relu("rp", "pl") + conv("d", "data", 8) + dropout("dr", "d")
    c16 = conv("c0", "data", 16)
    swap = lambda x, y: Wrong("two Concat members swapped", "cat", replace=(bottoms([x, y]), bottoms([y, x])))
    shifted = power("pw", "data", "pw", "shift: -0.5")
    return [
        Case("concat_views", members + concat("cat", ["a", "pl", "d"]) + conv1("u", "cat", 4), "conv_group:a+d {+pl} | relu:rp | conv:u", swap("a", "pl"),
             meta={"a": PLAIN, "d": PLAIN, "u": PLAIN}, alias={"a": ("cat", 0), "pl": ("cat", 8), "d": ("cat", 12)}, inputs="normal-1.45"),
        Case("concat_views_pooling_in_front", members + concat("cat", ["pl", "a", "d"]) + conv1("u", "cat", 4), "conv_group:a+d {+pl} | relu:rp | conv:u",
             Wrong("the pooling's ReLU over its neighbours", "cat", patch={"cat": lambda y, B: y.clamp(min=0)}),
             meta={"a": PLAIN, "d": PLAIN, "u": PLAIN}, alias={"pl": ("cat", 0), "a": ("cat", 4), "d": ("cat", 12)}, inputs="normal-1.45"),
        Case("concat_copy_second_reader", a + b + concat("cat", ["a", "b"]) + conv("v", "a", 8), "conv_group:a+b | copy:cat:a | copy:cat:b | conv:v", swap("a", "b"),
             meta={"a": PLAIN, "b": PLAIN, "v": PLAIN}, copy_concats=("cat",)),
        Case("concat_copy_six_channels", conv("a", "data", 6) + b + concat("cat", ["a", "b"]), "conv_group:a+b | copy:cat:a | copy:cat:b", swap("a", "b"),
             meta={"a": PLAIN, "b": PLAIN}, copy_concats=("cat",)),
        Case("concat_copy_one_bottom_twice", a + concat("cat", ["a", "a"]), "conv:a | copy:cat:a | copy:cat:a",
             Wrong("the second copy skipped", "cat", patch={"cat": lambda y, B: torch.cat([y[:, :8], 0 * y[:, 8:]], 1)}), meta={"a": PLAIN}, copy_concats=("cat",)),
        Case("concat_copy_net_input", a + concat("cat", ["data", "a"]), "conv:a | copy:cat:data | copy:cat:a", swap("data", "a"), meta={"a": PLAIN},
             copy_concats=("cat",)),
        Case("concat_copy_of_a_concat_top", a + b + c + concat("cat1", ["a", "b"]) + concat("cat", ["cat1", "c"]), "conv_group:a+b+c | copy:cat:cat1 | copy:cat:c",
             swap("cat1", "c"), meta={"a": PLAIN, "b": PLAIN, "c": PLAIN}, alias={"a": ("cat1", 0), "b": ("cat1", 8)}, copy_concats=("cat",)),
        Case("slice_views", c16 + slices("sl", "c0", ["s0", "s1"], 8) + conv1("v", "s0", 4) + pool("q", "s1", 3, 2) + concat("cat", ["s1", "s0"]),
             "conv:c0 | copy:cat:s1 | copy:cat:s0 | conv:v {+q}", Wrong("the two Slice tops swapped", "v", replace=('top: "s0" top: "s1"', 'top: "s1" top: "s0"')),
             meta={"c0": PLAIN, "v": PLAIN}, alias={"s0": ("c0", 0), "s1": ("c0", 8)}, copy_concats=("cat",)),
        Case("slice_copy_point_5", c16 + slices("sl", "c0", ["s0", "s1"], 5) + conv("v0", "s0", 4) + conv("v1", "s1", 4),
             "conv:c0 | copy:sl:s0 | copy:sl:s1 | conv_group:v0+v1", Wrong("the second copy from channel 0", "s1", patch={"s1": lambda y, B: B["c0"][:, :11]}),
             meta={"c0": PLAIN, "v0": PLAIN, "v1": PLAIN}, copy_slices=("sl",)),
        Case("slice_copy_eltwise_readers", c16 + slices("sl", "c0", ["s0", "s1"], 8) + elt("e", ["s0", "s1"], "operation: SUM coeff: 1 coeff: -0.5") +
             elt("m", ["s0", "s1"], "operation: MAX") + elt("pr", ["s0", "s1"], "operation: PROD") + unary("Softmax", "sm", "e", "sm"),
             "conv:c0 | copy:sl:s0 | copy:sl:s1 | eltwise:e | eltwise:m | eltwise:pr | softmax:sm",
             Wrong("the second copy from channel 0", "e", patch={"s1": lambda y, B: B["s0"]}), meta={"c0": PLAIN}, copy_slices=("sl",)),
        Case("slice_of_a_concat_view", a + b + concat("cat", ["a", "b"]) + slices("sl", "cat", ["s0", "s1"], 8) + conv1("v0", "s0", 4) + conv1("v1", "s1", 4),
             "conv_group:a+b | conv_group:v0+v1", Wrong("the two Slice tops swapped", "v0", replace=('top: "s0" top: "s1"', 'top: "s1" top: "s0"')),
             meta={n: PLAIN for n in ("a", "b", "v0", "v1")}, alias={"a": ("cat", 0), "b": ("cat", 8), "s0": ("cat", 0), "s1": ("cat", 8)}),
        Case("dropout_to_another_top", conv("c0", "data", 8) + dropout("dr", "c0", "d") + conv("v", "d", 8), "conv:c0 | conv:v",
             Wrong("a top of its own that nothing writes", "d", patch={"d": zero}), meta={"c0": PLAIN, "v": PLAIN}, alias={"d": ("c0", 0)}),
        Case("power_shift_folded", shifted + conv("c0", "pw", 8), "conv:c0", Wrong("the shift added to the padding", "c0", pad_value={"c0": -0.5}),
             meta={"c0": PLAIN}, alias={"pw": ("data", 0)}, shift={"pw": -0.5}, inputs="uniform"),
        Case("power_scale_launches", power("pw", "data", "pw", "shift: -0.5 scale: 2") + conv("c0", "pw", 8), "power:pw | conv:c0",
             Wrong("the scale ignored", "pw", replace=("scale: 2", "scale: 1")), meta={"c0": PLAIN}, inputs="uniform"),
        Case("power_input_with_a_second_reader", shifted + conv("c0", "pw", 8) + conv("v", "data", 8), "power:pw | conv:v | conv:c0",
             Wrong("the shift folded into an input that another layer reads", "v", patch={"data": lambda y, B: y - 0.5}), meta={"c0": PLAIN, "v": PLAIN},
             inputs="uniform"),
    ]


def batchnorm_cases():
    c0, u = conv("c0", "data", 8), conv("u", "c0", 8)
    in_place = bnorm("bn", "c0", "c0") + scale("sc", "c0", "c0")
    apart = bnorm("bn", "c0", "b") + scale("sc", "b", "s") + relu("r", "s", "r")
    stats = lambda phase: Wrong("%s statistics" % ("global" if phase == "TRAIN" else "batch"), "c0", bn_global={"bn": phase == "TRAIN"})
    out = []
    for phase in ("TEST", "TRAIN"):
        st = "bn_stats:bn | " if phase == "TRAIN" else ""
        kw = dict(phase=phase)
        out += [
            Case("bn_scale_relu_in_place", c0 + in_place + relu("r", "c0") + u, "conv:c0 | %sbn_apply:bn+sc+r | conv:u" % st, stats(phase),
                 meta={"c0": PLAIN, "u": PLAIN}, **kw),
            Case("bn_scale_relu_separate_tops", c0 + apart + conv("u", "r", 8), "conv:c0 | %sbn_apply:bn+sc+r | conv:u" % st,
                 Wrong("a middle blob at its zero fill", "b", patch={"b": zero}), meta={"c0": PLAIN, "u": PLAIN}, lazy=("b", "s"), **kw),
            Case("bn_chain_cut_by_a_second_consumer", c0 + apart + conv("v", "b", 8) + conv("u", "r", 8),
                 "conv:c0 | %sbn_apply:bn | bn_apply:sc+r | conv:v | conv:u" % st, Wrong("the BatchNorm top at its zero fill", "v", patch={"b": zero}),
                 meta={"c0": PLAIN, "u": PLAIN, "v": PLAIN}, lazy=("s",), **kw),
            Case("scale_relu_alone", c0 + scale("sc", "c0", "c0") + relu("r", "c0") + u, "conv:c0 | bn_apply:sc+r | conv:u",
                 Wrong("the ReLU omitted", "c0", replace=(relu("r", "c0"), "")), meta={"c0": PLAIN, "u": PLAIN}, **kw),
            Case("bn_chain_ended_by_a_leaky_relu", c0 + in_place + relu("r", "c0", slope=0.1) + u, "conv:c0 | %sbn_apply:bn+sc | relu:r | conv:u" % st,
                 Wrong("the slope dropped", "c0", replace=(" relu_param { negative_slope: 0.1 }", "")), meta={"c0": PLAIN, "u": PLAIN}, **kw),
        ]
    return out


def tail_cases():
    c0 = conv("c0", "data", 8) + relu("c0r", "c0")
    pa, pb = conv1("pa", "c0", 32) + relu("par", "pa"), conv("pb", "c0", 32) + relu("pbr", "pb")
    cat = concat("cat", ["pa", "pb"])
    h1, h2 = conv1("h1", "cat", 4), conv1("h2", "cat", 16) + sigmoid("sg", "h2", "sg")
    half = lambda k=32: Wrong("a head's sum over one producer only", "h1", patch={"cat": lambda y, B: torch.cat([y[:, :k], 0 * y[:, k:]], 1)})
    views = {"pa": ("cat", 0), "pb": ("cat", 32)}
    base = {"c0": FUSED, "pa": FUSED, "pb": FUSED, "h1": PLAIN}
    two = dict(base, h2=(False, "sg"))
    return [Case(*a, alias=kw.pop("alias", views), tail=True, **kw) for a, kw in [
        (("tail_one_level_two_heads", c0 + pa + pb + cat + h1 + h2, "conv:c0 | conv_group:pa+pb {tail: h1+h2}", half()), dict(meta=two)),
        (("tail_two_levels", c0 + pa + conv1("m", "c0", 8) + relu("mr", "m") + conv("pb", "m", 32) + relu("pbr", "pb") + cat + h1 + h2,
          "conv:c0 | conv_group:pa+m {partial sums of h1+h2} | conv:pb {tail: h1+h2}", half()), dict(meta=dict(two, m=FUSED))),
        (("tail_one_head", c0 + pa + pb + cat + h1, "conv:c0 | conv_group:pa+pb {tail: h1}", half()), dict(meta=base)),
        (("tail_four_heads", c0 + pa + pb + cat + h1 + conv1("h2", "cat", 4) + conv1("h3", "cat", 8) + sigmoid("sg", "h3", "sg") + conv1("h4", "cat", 4),
          "conv:c0 | conv_group:pa+pb {tail: h1+h2+h3+h4}", half()), dict(meta=dict(base, h2=PLAIN, h3=(False, "sg"), h4=PLAIN))),
        (("tail_refused_16_channel_producer", c0 + conv1("pa", "c0", 16) + relu("par", "pa") + conv("pb", "c0", 48) + relu("pbr", "pb") + cat + h1 + h2,
          "conv:c0 | conv_group:pa+pb | conv_group:h1+h2", half(16)), dict(meta=two, alias={"pa": ("cat", 0), "pb": ("cat", 16)})),
        (("tail_refused_3_output_head", c0 + pa + pb + cat + conv1("h1", "cat", 3) + h2, "conv:c0 | conv_group:pa+pb | conv_group:h1+h2", half()), dict(meta=two)),
        (("tail_refused_pooling_writes_part", conv("c0", "data", 32) + pa + pool("pb", "c0", 3, 1, 1) + cat + h1 + h2,
          "conv:c0 | conv:pa {+pb} | conv_group:h1+h2", half()), dict(meta={"c0": PLAIN, "pa": FUSED, "h1": PLAIN, "h2": (False, "sg")})),
        (("tail_refused_3x3_head", c0 + pa + pb + cat + conv("h1", "cat", 4) + h2, "conv:c0 | conv_group:pa+pb | conv_group:h1+h2", half()), dict(meta=two)),
    ]]


CASES = epilogue_cases() + level_cases() + pool_lrn_cases() + view_cases() + batchnorm_cases() + tail_cases()
IDS = ["%s%s" % (c.name, "_train" if c.phase == "TRAIN" else "") for c in CASES]
assert len(set(IDS)) == len(IDS)


# ---------------------------------------------------------------------------------------------------------------------- the reference
def parse(text, phase):
    msg = proto.parse_text(text)
    spec = NetSpec(msg, phase)
    spec.infer()
    return msg, spec


def numpy_blobs(B):
    return {k: v.detach().numpy().astype(np.float64) for k, v in B.items()}


@functools.lru_cache(maxsize=None)
def reference(index):
    """The float64 forward of case `index`, computed once and shared by the tests: the parameters and the input the engine gets, every
    blob, what every layer read, the two largest values of every MAX pooling window."""
    case = CASES[index]
    msg, spec = parse(case.text, case.phase)
    params = random_params(spec, case.seed)
    rng = np.random.default_rng([case.seed, 1])      # (not the stream the parameters were drawn from)
    shape = spec.input_shapes["data"]
    x = rng.random(shape) if case.inputs == "uniform" else rng.standard_normal(shape) + (float(case.inputs[6:]) if case.inputs != "normal" else 0.0)
    x = {"data": x.astype(np.float32)}
    B, first, seen, top2 = forward_net(spec, as_torch(params), x)
    return dict(msg=msg, spec=spec, params=params, x=x, blobs=numpy_blobs(B), seen={k: v.numpy() for k, v in seen.items()},
                top2={k: v.numpy() for k, v in top2.items()})


# ------------------------------------------------------------------------------------- without a GPU: the interpreter, and the cases can fail
def test_interpreter_layer_types_by_hand():
    """Power, Slice, Dropout, Softmax and the Eltwise operations of forward_net against their formulas in numpy."""
    text = ('input: "data" input_shape { dim: 2 dim: 6 dim: 3 dim: 2 }\n' + power("pw", "data", "pw", "power: 2 scale: 3 shift: -0.5") +
            slices("sl", "pw", ["s0", "s1", "s2"], 2).replace("slice_point: 2", "slice_point: 2 slice_point: 4") + dropout("dr", "s0", "d") +
            elt("e", ["d", "s1", "s2"], "operation: SUM coeff: 1 coeff: -0.5 coeff: 2") + elt("m", ["d", "s1", "s2"], "operation: MAX") +
            elt("pr", ["d", "s1", "s2"], "operation: PROD") + unary("Softmax", "sm", "e", "sm") +
            'layer { name: "sq" type: "Slice" bottom: "data" top: "q0" top: "q1" top: "q2" }\n')
    _, spec = parse(text, "TEST")
    x = np.random.default_rng(3).standard_normal((2, 6, 3, 2))
    B = numpy_blobs(forward_net(spec, {}, {"data": x})[0])
    pw = (3 * x - 0.5) ** 2
    s0, s1, s2 = pw[:, :2], pw[:, 2:4], pw[:, 4:]
    e = s0 - 0.5 * s1 + 2 * s2
    ex = np.exp(e - e.max(axis=1, keepdims=True))
    for name, want in (("pw", pw), ("s0", s0), ("s1", s1), ("s2", s2), ("d", s0), ("e", e), ("m", np.maximum(np.maximum(s0, s1), s2)), ("pr", s0 * s1 * s2),
                       ("sm", ex / ex.sum(axis=1, keepdims=True)), ("q0", x[:, :2]), ("q1", x[:, 2:4]), ("q2", x[:, 4:])):
        assert B[name].shape == want.shape and np.allclose(B[name], want, rtol=1e-13, atol=1e-13), name
    with pytest.raises(AssertionError):      # Dropout in TRAIN draws a mask
        forward_net(parse(text, "TRAIN")[1], {}, {"data": x})


def test_interpreter_keeps_what_in_place_layers_overwrote():
    index = IDS.index("convolution_reader_ahead_of_the_relu")
    ref = reference(index)
    B, first, seen, _ = forward_net(ref["spec"], as_torch(ref["params"]), ref["x"])
    assert np.array_equal(B["c0"].numpy(), np.maximum(first["c0"].numpy(), 0)) and (first["c0"].numpy() < 0).any()
    assert seen["s"] is first["c0"] and seen["u"] is B["c0"] and seen["r0"] is first["c0"]


def test_a_blob_that_a_layer_reads_is_no_output():
    """Why "the middle blob is a net output" is no case of the matrix."""
    for index, case in enumerate(CASES):
        spec = reference(index)["spec"]
        assert not set(spec.output_blobs()) & {b for l in spec.layers for b in l.bottoms}, case.name


def wrong_blobs(case, ref):
    w = case.wrong
    spec = ref["spec"]
    if w.replace is not None:
        assert case.text.count(w.replace[0]) == 1, w.replace[0]
        spec = parse(case.text.replace(*w.replace), case.phase)[1]
    assert w.replace or w.patch or w.pad_value or w.bn_global
    return numpy_blobs(forward_net(spec, as_torch(ref["params"]), ref["x"], patch=w.patch, pad_value=w.pad_value, bn_global=w.bn_global)[0])


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_reference_shows_the_case_can_fail(index):
    case, ref = CASES[index], reference(index)
    blobs, spec = ref["blobs"], ref["spec"]
    assert set(blobs) == set(spec.blob_shapes)
    # the wrong evaluation is a hundred thresholds away, on a blob the GPU test compares
    err = rel_err(wrong_blobs(case, ref)[case.wrong.blob], blobs[case.wrong.blob])
    assert err >= WRONG_AT_LEAST, (case.wrong.what, err)
    # float32 rounding of the same net is a tenth of the threshold
    B32 = numpy_blobs(forward_net(spec, as_torch(ref["params"], dtype=torch.float32), ref["x"], dtype=torch.float32)[0])
    for name, want in blobs.items():
        assert rel_err(B32[name], want) < F32_AT_MOST, (name, rel_err(B32[name], want))
    # the inputs: every ReLU reads a tenth of its elements on each side of zero, no MAX pooling window holds a tie
    for l in spec.layers:
        if l.type == "ReLU":
            negative = (ref["seen"][l.name] < 0).mean()
            assert 0.1 <= negative <= 0.9, (l.name, negative)
    for name, two in ref["top2"].items():
        assert not (two[..., 0] == two[..., 1]).any(), name


# ------------------------------------------------------------------------------------------------------------------- on the GPU
def launch_list(eng):
    return [(op.kind, re.sub(r" \[[^\]]*\]", "", op.name)) for op in eng.ops]


def make_engine(case, ref, **kw):
    from fcn_object_detector_amd.engine import Engine
    eng = Engine(NetSpec(ref["msg"], case.phase), params={k: [a.copy() for a in v] for k, v in ref["params"].items()}, device=0, autotune=False, **kw)
    eng.host_array("data")[...] = ref["x"]["data"]
    return eng


def compare(eng, ref, names, worst):
    for name in names:
        got, want = eng.read_blob(name), ref["blobs"][name]
        assert got.shape == want.shape, name
        worst[name] = max(worst.get(name, 0.0), rel_err(got, want))
        assert worst[name] < TOL, (name, worst[name])
        assert elem_err(got, want, TOL)[0] <= 1, (name, elem_err(got, want, TOL))


def same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def copies(out):
    return {k: np.array(v, np.float32) for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_forward_plan_path(gpu, monkeypatch, index):
    case, ref = CASES[index], reference(index)
    if case.tail:
        monkeypatch.setenv("FCN_CONV_TAIL", "1")
    names = list(ref["spec"].blob_shapes)
    worst = {}
    eng = make_engine(case, ref)
    try:
        # 1. the path
        assert launch_list(eng) == case.launches
        assert eng._conv_layer_meta == {k: dict(relu=r, sigmoid_top=s) for k, (r, s) in case.meta.items()}
        assert (eng.alias, eng.shift) == (case.alias, case.shift)
        assert (eng.copy_concats, eng.copy_slices, set(eng._lazy_blob_ops)) == (set(case.copy_concats), set(case.copy_slices), set(case.lazy))
        for top, sh in case.shift.items():      # the upload adds the shift; the input reads back without it, the Power top with it
            assert eng.blobs[eng.alias[top][0]].upload_shift == sh
        # 2. and 3.: the lazy blobs ahead of the others, a forward behind them, the lazy blobs behind the others, a forward without a graph
        plain = [n for n in names if n not in case.lazy]
        first = copies(eng.forward())
        assert set(first) == set(ref["spec"].output_blobs()) - set(ref["spec"].mask_blobs)
        compare(eng, ref, list(case.lazy) + plain, worst)
        again = copies(eng.forward())
        assert same_bits(first, again)
        compare(eng, ref, plain + list(case.lazy), worst)
        assert same_bits(first, copies(eng.forward()))
        assert same_bits(first, copies(eng.forward(use_graph=False)))
    finally:
        eng.close()
    for kw in (dict(fuse=False, group_convs=False), dict(fuse=True, group_convs=False)):
        eng = make_engine(case, ref, **kw)
        try:
            eng.forward()
            compare(eng, ref, names, worst)
        finally:
            eng.close()
    print("PLANPATH %s %s" % (IDS[index], " ".join("%s %.2g" % kv for kv in worst.items())))
