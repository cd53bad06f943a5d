"""The backward planner's accumulate paths, emitter by emitter: a blob with two consumers, the layer under test as one of them.

Template (the recipe of tests/test_gpu_classifier_nets._small_step: TrainEngine, base_lr 0, no autotuner, one step, float64 autograd):

    data (2 x 3 x 11 x 10), label (2)
    c0  = Convolution(data) 3x3 pad 1, C outputs, learns            <- the blob whose gradient has two writers
    t   = T(c0), NOT in place;  fa = InnerProduct(t) -> 4
    s   = Convolution(c0) 3x3, 5 outputs;  fs = InnerProduct(s) -> 4
    sum = Eltwise SUM(fa, fs);  loss = SoftmaxWithLoss(sum, label)

C = 8 where the emitter wants 16-byte aligned views, else 6 in pixels of 8 floats.  The layer listed FIRST runs its backward SECOND and
adds into dc0 (order "t_first": T takes its accumulate path; "s_first": T writes, s's data gradient accumulates).  relu_on_c0 (both orders) puts an
in-place ReLU behind c0, fused into its epilogue: dc0 = mask * (dT + dS), the mask folded into the last writer where that is a
data-gradient record or a MAX pooling and a launch of its own behind every other writer.  Every case reads from eng.bwd_ops that the
intended launches ran in the intended order.

The part without a GPU (the tests not marked gpu) shows on the reference alone that each case CAN fail: both writers contribute at
least 5 % of dc0, the ReLU masks a tenth of c0 and leaves a tenth, the un-masked sum is non-zero under the mask, the leaky cases have a
tenth of their elements on the negative side, and no MAX pooling window holds a tie.

Thresholds: tests/test_gpu_classifier_nets.py's, rel_err < 1e-4 for blob gradients and < 5e-4 for parameter gradients."""
import functools
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from conftest import rel_err
from fcn_object_detector_amd import proto
from fcn_object_detector_amd.netspec import NetSpec
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from test_gpu_classifier_nets import inputs_for
from torch_fanout_ref import as_torch, random_params, torch_net

FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'
HEAD = 'input: "data" input_shape { dim: 2 dim: 3 dim: 11 dim: 10 }\ninput: "label" input_shape { dim: 2 }\n'
FROZEN = "param { lr_mult: 0 } param { lr_mult: 0 }"
S_WRITER = ("dgrad", "s")


def conv(name, bottom, n, geometry="kernel_size: 3", head=""):
    return 'layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" %s convolution_param { num_output: %d %s %s } }\n' % (
        name, bottom, name, head, n, geometry, FILL)


def fc(name, bottom, n=4):
    return 'layer { name: "%s" type: "InnerProduct" bottom: "%s" top: "%s" inner_product_param { num_output: %d %s } }\n' % (name, bottom, name, n, FILL)


def relu(name, blob, top=None, slope=None):
    return 'layer { name: "%s" type: "ReLU" bottom: "%s" top: "%s"%s }\n' % (
        name, blob, top or blob, "" if slope is None else " relu_param { negative_slope: %g }" % slope)


def tail(tops):
    return 'layer { name: "sum" type: "Eltwise" %s top: "sum" eltwise_param { operation: SUM } }\n' % " ".join('bottom: "%s"' % t for t in tops) + \
        'layer { name: "loss" type: "SoftmaxWithLoss" bottom: "sum" bottom: "label" top: "loss" }\n'


MAXPOOL = 'layer { name: "%s" type: "Pooling" bottom: "%s" top: "%s"%s pooling_param { pool: MAX kernel_size: %d stride: 2%s } }\n'
BN = 'layer { name: "t" type: "BatchNorm" bottom: "FAN" top: "t"%s }\n' \
     'layer { name: "t_sc" type: "Scale" bottom: "t" top: "t" scale_param { bias_term: true } }\n'


@dataclass(frozen=True)
class Case:
    """One layer under test.  t: the layers of the T branch, from the blob FAN (of C channels) to the blob "t"; writer: (kind, name) of the
    launch that writes T's share of d(FAN); folds: that launch is a record the ReLU mask of c0 folds into when it is the last writer;
    types: the keys of the planner's tables the case runs; params: layers whose parameter gradients are compared beside c0's;
    pre: layers ahead of c0; gain: see below; mid: layers between c0 and the branches (then `fan` names the blob with two consumers)."""
    name: str
    types: tuple
    t: str
    writer: tuple
    c: int = 6
    folds: bool = False
    params: tuple = ()
    pre: str = ""
    c0_bottom: str = "data"
    mid: str = ""
    fan: str = "c0"
    also: tuple = ()      # further (kind, name) launches the T branch must show
    gain: tuple = ()      # (layer, factor) on the weights random_params drew: where a branch would otherwise fall below 5 % of dc0


def _tconv(name, geometry, group="", head=""):
    return 'layer { name: "%s" type: "Deconvolution" bottom: "FAN" top: "%s" %s convolution_param { num_output: %s %s %s %s } }\n' % (
        name, name, head, "%s", group, geometry, "%s")


CASES = [
    Case("max_pooling", ("Pooling",), MAXPOOL % ("t", "FAN", "t", "", 3, " pad: 1"), ("maxpool_bwd", "t"), folds=True),
    Case("ave_pooling", ("Pooling",), 'layer { name: "t" type: "Pooling" bottom: "FAN" top: "t" pooling_param { pool: AVE kernel_size: 3 stride: 2 pad: 1 } }\n',
         ("avepool_bwd", "t"), c=8),
    Case("ave_pooling_global", ("Pooling",), 'layer { name: "t" type: "Pooling" bottom: "FAN" top: "t" pooling_param { pool: AVE global_pooling: true } }\n',
         ("avepool_bwd", "t"), c=8, gain=(("fa", 4.0),)),      # (each pixel gets 1 / 110 of the pooled gradient)
    Case("lrn", ("LRN",), 'layer { name: "t" type: "LRN" bottom: "FAN" top: "t" lrn_param { local_size: 5 alpha: 0.5 beta: 0.75 } }\n', ("lrn_bwd", "t")),
    # a ReLU of its own behind a pooling: no convolution epilogue can take it
    Case("relu_plain", ("ReLU",), relu("t", "FAN", "t"), ("relu_bwd", "t"), mid=MAXPOOL % ("p0", "c0", "p0", "", 2, ""), fan="p0", folds=True),
    Case("sigmoid_plain", ("Sigmoid",), 'layer { name: "t" type: "Sigmoid" bottom: "FAN" top: "t" }\n', ("sigmoid_bwd", "t")),
    # the Sigmoid that rides in the epilogue of the convolution ct (its only consumer): _sigmoid's own branch; ct's data gradient writes dc0
    Case("sigmoid_fused", ("Sigmoid", "Convolution"), conv("ct", "FAN", 6, "kernel_size: 1") + 'layer { name: "t" type: "Sigmoid" bottom: "ct" top: "t" }\n',
         ("dgrad", "ct"), folds=True, params=("ct",), also=(("sigmoid_bwd", "t"),)),
    Case("crop", ("Crop",), 'layer { name: "t" type: "Crop" bottom: "FAN" bottom: "small" top: "t" crop_param { axis: 2 offset: 1 } }\n', ("crop_bwd", "t"),
         pre='layer { name: "small" type: "Pooling" bottom: "data" top: "small" pooling_param { pool: MAX kernel_size: 3 stride: 1 } }\n'),
    Case("interp", ("Interp",), 'layer { name: "t" type: "Interp" bottom: "FAN" top: "t" interp_param { zoom_factor: 2 } }\n', ("interp_bwd", "t")),
    # the SegNet form: c0 works at the pooled size, the mask is the second top of the pooling ahead of it
    Case("upsample", ("Upsample",), 'layer { name: "t" type: "Upsample" bottom: "FAN" bottom: "pe_mask" top: "t" upsample_param { upsample_h: 11 upsample_w: 10 } }\n',
         ("unpool_bwd", "t"), pre=conv("e0", "data", 6, "kernel_size: 3 pad: 1") + MAXPOOL % ("pe", "e0", "pe", ' top: "pe_mask"', 2, ""), c0_bottom="pe"),
    Case("deconvolution_depthwise", ("Deconvolution",),
         _tconv("t", "kernel_size: 4 stride: 2 pad: 1 bias_term: false", "group: 6", "param { lr_mult: 0 }") % (6, 'weight_filler { type: "bilinear" }'),
         ("deconv_bwd", "t")),
    Case("deconvolution_dense", ("Deconvolution",), _tconv("t", "kernel_size: 4 stride: 2 pad: 1") % (5, FILL), ("dgrad", "t"), c=8, folds=True, params=("t",)),
    Case("batchnorm_chain", ("BatchNorm", "Scale"), BN % "" + relu("t_relu", "t"), ("bn_bwd_apply", "t"), c=8, params=("t_sc",), also=(("bn_bwd_reduce", "t"),)),
    Case("batchnorm_chain_global_stats", ("BatchNorm", "Scale"), BN % " batch_norm_param { use_global_stats: true }" + relu("t_relu", "t"),
         ("bn_bwd_apply", "t"), c=8, params=("t_sc",), also=(("bn_bwd_reduce", "t"),)),
    Case("scale_alone", ("Scale",), 'layer { name: "t" type: "Scale" bottom: "FAN" top: "t" scale_param { bias_term: true } }\n', ("bn_bwd_apply", "t"),
         c=8, params=("t",), also=(("bn_bwd_reduce", "t"),)),
    Case("convolution_stride1", ("Convolution",), conv("t", "FAN", 7, "kernel_size: 3 pad: 1"), ("dgrad", "t"), folds=True, params=("t",)),
    Case("convolution_strided", ("Convolution",), conv("t", "FAN", 7, "kernel_size: 3 stride: 2 pad: 1"), ("tconv_dgrad", "t"), folds=True, params=("t",)),
    Case("convolution_grouped", ("Convolution",), conv("t", "FAN", 8, "kernel_size: 3 pad: 1 group: 2"), ("dgrad", "t"), c=8, folds=True, params=("t",)),
    Case("convolution_dilated", ("Convolution",), conv("t", "FAN", 7, "kernel_size: 3 pad: 2 dilation: 2"), ("dconv_dgrad", "t"), folds=True, params=("t",)),
    Case("convolution_rectangular", ("Convolution",), conv("t", "FAN", 7, "kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 1"), ("rconv_dgrad", "t"), folds=True,
         params=("t",)),
    Case("convolution_depthwise", ("DepthwiseConvolution",),
         'layer { name: "t" type: "DepthwiseConvolution" bottom: "FAN" top: "t" convolution_param { num_output: 6 kernel_size: 3 pad: 1 %s } }\n' % FILL,
         ("dwconv_dgrad", "t"), folds=True, params=("t",)),
    Case("inner_product", ("InnerProduct",), fc("t", "FAN", 7), ("inner_product_bwd", "t"), params=("t",)),
    # T hands its own gradient to two bottoms: c0, already written in the order t_first (the add), and o, which is not (the copy)
    Case("eltwise_sum", ("Eltwise",), 'layer { name: "t" type: "Eltwise" bottom: "FAN" bottom: "o" top: "t" eltwise_param { operation: SUM } }\n',
         ("eltwise_bwd", "t:c0"), pre=conv("o", "data", 6, "kernel_size: 3 pad: 1"), params=("o",), also=(("eltwise_bwd", "t:o"),)),
    # a Concat that copies (c0 has another consumer) and hands each member its channels of dY: c0 already holds a gradient, o does not
    Case("concat_copy", ("Concat",), 'layer { name: "t" type: "Concat" bottom: "FAN" bottom: "o" top: "t" }\n',
         ("concat_bwd", "t:c0"), pre=conv("o", "data", 6, "kernel_size: 3 pad: 1"), params=("o",), also=(("concat_bwd", "t:o"),)),
]
BY_NAME = {c.name: c for c in CASES}
VARIANTS = [("t_first", False), ("s_first", False), ("t_first", True), ("s_first", True)]      # (order, relu_on_c0)


def net_text(case, order, relu_on_c0):
    t_branch = case.t.replace("FAN", case.fan) + fc("fa", "t")
    s_branch = conv("s", case.fan, 5) + fc("fs", "s")
    return HEAD + case.pre + conv("c0", case.c0_bottom, case.c, "kernel_size: 3 pad: 1") + (relu("r0", "c0") if relu_on_c0 else "") + case.mid + \
        (t_branch + s_branch if order == "t_first" else s_branch + t_branch) + tail(["fa", "fs"])


# ---- the cases beside the matrix: three consumers, and ReLU layers with a negative slope of 0.1 (never fused: launches of their own)
THREE = HEAD + conv("c0", "data", 6, "kernel_size: 3 pad: 1") + MAXPOOL % ("t", "c0", "t", "", 3, " pad: 1") + fc("fa", "t") + \
    'layer { name: "n" type: "LRN" bottom: "c0" top: "n" lrn_param { local_size: 5 alpha: 0.5 beta: 0.75 } }\n' + fc("fb", "n") + \
    conv("s", "c0", 5) + fc("fs", "s") + tail(["fa", "fb", "fs"])
_C0 = HEAD + conv("c0", "data", 6, "kernel_size: 3 pad: 1")
_P0 = MAXPOOL % ("p0", "c0", "p0", "", 2, "")
_C8 = HEAD + conv("c0", "data", 8, "kernel_size: 3 pad: 1")
_A0 = 'layer { name: "p0" type: "Pooling" bottom: "c0" top: "p0" pooling_param { pool: AVE kernel_size: 2 stride: 2 } }\n'      # (half its outputs are negative)
_ONE = 'layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fa" bottom: "label" top: "loss" }\n'
# name -> (net, the ReLU layer, the blob with two consumers or "c0", blobs whose gradients are compared, branch tops, launches in order)
LEAKY = {
    "after_pooling": (_C8 + _A0 + relu("t", "p0", "t", 0.1) + fc("fa", "t") + _ONE, "t", "c0", ("p0", "c0"), ("fa",), [("relu_bwd", "t")]),
    "in_place_after_convolution": (_C0 + conv("ct", "c0", 6, "kernel_size: 3 pad: 1") + relu("t", "ct", None, 0.1) + fc("fa", "ct") + _ONE, "t", "c0",
                                   ("ct", "c0"), ("fa",), [("relu_bwd", "t"), ("dgrad", "ct")]),
    "after_pooling_fan_out": (_C8 + _A0 + relu("t", "p0", "t", 0.1) + fc("fa", "t") + conv("s", "p0", 5) + fc("fs", "s") + tail(["fa", "fs"]), "t", "p0",
                              ("p0", "c0"), ("fa", "fs"), [S_WRITER, ("relu_bwd", "t")]),
    # the in-place leaky ReLU sits on the blob with two writers: its launch rewrites the SUM; the MAX pooling that wrote last takes no mask
    "in_place_under_fan_out": (_C0 + relu("t", "c0", None, 0.1) + MAXPOOL % ("m", "c0", "m", "", 3, " pad: 1") + fc("fa", "m") + conv("s", "c0", 5) +
                               fc("fs", "s") + tail(["fa", "fs"]), "t", "c0", ("c0",), ("fa", "fs"), [S_WRITER, ("maxpool_bwd", "m"), ("relu_bwd", "t")]),
    # behind BatchNorm + Scale: the chain ends in front of a ReLU with a slope.  (The branch s keeps the gradient of c0's bias away from the
    # exact zero a convolution under batch statistics alone would have.)
    "behind_batchnorm_chain": (_C8 + (BN % "").replace("FAN", "c0") + relu("t_relu", "t", None, 0.1) + fc("fa", "t") + conv("s", "c0", 5) + fc("fs", "s") +
                               tail(["fa", "fs"]), "t_relu", "c0", ("c0",), ("fa", "fs"), [S_WRITER, ("relu_bwd", "t_relu"), ("bn_bwd_apply", "t")]),
}


# ---------------------------------------------------------------------------------------------------------------------- the reference
def parse(text):
    msg = proto.parse_text(text)
    spec = NetSpec(msg, "TRAIN")
    spec.infer()
    return msg, spec


@functools.lru_cache(maxsize=None)
def reference(text, fan="c0", branches=("fa", "fs"), seed=1, gain=()):
    """One float64 forward and backward of the net, computed once per net and shared by the tests: the parameters and inputs the engine
    gets, the loss, the gradient of every blob at the value its layer WROTE (under an in-place ReLU: the convolution's output), the
    parameter gradients, the share of every branch in the gradient of `fan` at its FINAL value (the un-masked terms), and the two
    largest values of every MAX pooling window."""
    msg, spec = parse(text)
    params = random_params(spec, seed)
    for layer, factor in gain:
        params[layer][0] *= np.float32(factor)
    x = inputs_for(spec, 0, classes=4)
    P = as_torch(params, grad=True)
    top2 = {}
    B, first, seen = torch_net(spec, P, x, top2=top2)
    blobs = [n for n, v in B.items() if isinstance(v, torch.Tensor) and v.requires_grad and n != "total_loss"]
    wrote = {n: first.get(n, B[n]) for n in blobs}
    leaves = [p for v in P.values() for p in v if p.requires_grad]
    grads = torch.autograd.grad(B["total_loss"], [wrote[n] for n in blobs] + leaves, retain_graph=True, allow_unused=True)
    dblob = {n: g.numpy() for n, g in zip(blobs, grads) if g is not None}
    relus = [l for l in spec.layers if l.type == "ReLU"]      # what every ReLU layer read, and the gradient it hands down
    drelu = torch.autograd.grad(B["total_loss"], [seen[l.name] for l in relus], retain_graph=True) if relus else ()
    relu_in = {l.name: (seen[l.name].detach().numpy(), g.numpy()) for l, g in zip(relus, drelu)}
    it = iter(grads[len(blobs):])
    dparam = {k: [next(it).numpy() if p.requires_grad else None for p in v] for k, v in P.items()}
    if len(branches) > 1:
        dsum = torch.autograd.grad(B["total_loss"], B["sum"], retain_graph=True)[0]
        shares = [torch.autograd.grad(B[b], B[fan], grad_outputs=dsum, retain_graph=True)[0].numpy() for b in branches]
    else:
        shares = [torch.autograd.grad(B["total_loss"], B[fan], retain_graph=True)[0].numpy()]
    return dict(msg=msg, spec=spec, params=params, x=x, loss=float(B["total_loss"].detach()), dblob=dblob, dparam=dparam, shares=shares,
                wrote={n: v.detach().numpy() for n, v in wrote.items()}, relu_in=relu_in, top2={k: v.numpy() for k, v in top2.items()})


def assert_no_ties(ref, relu_on=()):
    """No MAX pooling window with two equal maxima.  Behind an in-place ReLU whole windows are 0: there every candidate is a masked
    element, whose gradient the mask removes whichever the pooling names - only ties at a positive value would matter."""
    pools = {l.name: l for l in ref["spec"].layers if l.type == "Pooling"}
    for name, two in ref["top2"].items():
        tie = two[..., 0] == two[..., 1]
        if pools[name].bottoms[0] in relu_on:
            tie &= two[..., 0] > 0
        assert not tie.any(), "MAX pooling %s: %d windows hold a tie" % (name, int(tie.sum()))


def assert_both_writers_count(ref):
    total = np.abs(sum(ref["shares"])).max()
    for i, s in enumerate(ref["shares"]):
        assert np.abs(s).max() >= 0.05 * total, "branch %d contributes %.3g of %.3g" % (i, np.abs(s).max(), total)


# ------------------------------------------------------------------------------------------ without a GPU: the cases can fail
@pytest.mark.parametrize("order,relu_on_c0", VARIANTS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_shows_both_writers_and_the_mask(case, order, relu_on_c0):
    ref = reference(net_text(case, order, relu_on_c0), case.fan, gain=case.gain)
    assert_no_ties(ref, ("c0",) if relu_on_c0 else ())
    assert_both_writers_count(ref)
    if relu_on_c0:
        masked = ref["wrote"]["c0"] <= 0
        assert 0.1 <= masked.mean() <= 0.9, masked.mean()
        if case.fan == "c0":      # "mask the sum" and "mask the last term" differ only where the un-masked sum is non-zero under the mask
            assert np.abs(sum(ref["shares"]))[masked].max() > 0.05 * np.abs(sum(ref["shares"])).max()
            assert np.allclose(ref["dblob"]["c0"], np.where(masked, 0.0, sum(ref["shares"])), rtol=1e-12, atol=0.0)


def test_reference_of_the_three_consumer_case():
    ref = reference(THREE, "c0", ("fa", "fb", "fs"))
    assert_no_ties(ref)
    assert_both_writers_count(ref)


@pytest.mark.parametrize("which", sorted(LEAKY))
def test_reference_of_the_leaky_cases(which):
    text, layer, fan, _, branches, _ = LEAKY[which]
    ref = reference(text, fan, branches)
    assert_no_ties(ref)
    assert_both_writers_count(ref)
    x, dx = ref["relu_in"][layer]
    negative = x < 0
    assert 0.1 <= negative.mean() <= 0.9, negative.mean()
    # the slope term is visible: the gradient on the negative side is a tenth of dY, not zero (the plain mask)
    assert np.abs(dx[negative]).max() > 0.01 * np.abs(dx).max()


# ------------------------------------------------------------------------------------------------------------------- on the GPU
def launches(eng, wanted):
    """(kind, name) of the backward launches among `wanted`, in their order (a launch's label may carry its geometry behind the name)."""
    got = [(op.kind, op.name.split(" ")[0]) for op in eng.bwd_ops]
    return [kn for kn in got if kn in wanted]


def step_and_compare(text, ref, blobs, layers):
    """The recipe of tests/test_gpu_classifier_nets._small_step; returns the engine (the caller closes it)."""
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(ref["msg"], "TRAIN"), dict(ref["spec"].input_shapes), params={k: [a.copy() for a in v] for k, v in ref["params"].items()},
                      device=0, solver=sp, autotune=False)
    for k, v in ref["x"].items():
        eng.host_array(k)[...] = v
    out = eng.step(seed=1)
    assert abs(out["loss"] - ref["loss"]) < 1e-4 * abs(ref["loss"]), (out["loss"], ref["loss"])
    worst = {}
    for name in blobs:
        worst[name] = rel_err(eng.read_grad(name), ref["dblob"][name])
    got = eng.download_grads()
    for name in layers:
        for i, (g, r) in enumerate(zip(got[name], ref["dparam"][name])):
            assert g.shape == r.shape, name
            worst["%s[%d]" % (name, i)] = rel_err(g, r)
    print("FANOUT", " ".join("%s %.3g" % kv for kv in worst.items()))
    for key, err in worst.items():
        assert err < (5e-4 if "[" in key else 1e-4), (key, err)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("order,relu_on_c0", VARIANTS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_two_writers_of_one_gradient(gpu, case, order, relu_on_c0):
    text = net_text(case, order, relu_on_c0)
    ref = reference(text, case.fan, gain=case.gain)
    eng = step_and_compare(text, ref, sorted({"c0", case.fan}), ("c0", "s") + case.params)
    try:
        mask = ("relu_bwd", "c0")
        got = launches(eng, (case.writer, S_WRITER, mask) + case.also)
        writers = [kn for kn in got if kn in (case.writer, S_WRITER)]
        assert writers == ([S_WRITER, case.writer] if order == "t_first" else [case.writer, S_WRITER]), got
        assert all(kn in got for kn in case.also), got
        if relu_on_c0:      # the mask rides in the last writer where it can (s's data gradient always can), and is the launch behind it where it cannot
            assert (mask in got) == (order == "t_first" and not case.folds), got
            assert mask not in got or got.index(mask) > max(got.index(w) for w in writers), got
    finally:
        eng.close()


@pytest.mark.gpu
def test_three_writers_of_one_gradient(gpu):
    """c0 feeds a MAX pooling, an LRN and a convolution: the accumulate path is taken twice."""
    ref = reference(THREE, "c0", ("fa", "fb", "fs"))
    eng = step_and_compare(THREE, ref, ["c0"], ("c0", "s"))
    try:
        assert launches(eng, (S_WRITER, ("lrn_bwd", "n"), ("maxpool_bwd", "t"))) == [S_WRITER, ("lrn_bwd", "n"), ("maxpool_bwd", "t")]
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(LEAKY))
def test_relu_with_a_negative_slope(gpu, which):
    """negative_slope 0.1: dX = dY where the output is positive and 0.1 dY elsewhere, in a launch of the ReLU layer's own - no epilogue, no
    BatchNorm chain and no pooling backward carries such a mask (the forward shows the layer as a launch of its own as well)."""
    text, layer, fan, blobs, branches, order = LEAKY[which]
    ref = reference(text, fan, branches)
    learn = [l.name for l in ref["spec"].param_layers() if l.type != "BatchNorm"]
    eng = step_and_compare(text, ref, blobs, learn)
    try:
        assert launches(eng, order) == order
        assert ("relu", layer) in [(op.kind, op.name) for op in eng.ops]
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------ refusals, by layer name
_O = conv("o", "data", 6, "kernel_size: 3 pad: 1")
_S = conv("s", "c0", 5) + fc("fs", "s")
_ELT = 'layer { name: "t" type: "Eltwise" bottom: "c0" bottom: "%s" top: "t" eltwise_param { operation: %s } }\n'
# condition -> (layer type, net, what the message says); tests/test_backward_ledger.py holds its REFUSES to these
REFUSALS = {
    "Dropout into an already written gradient": (
        "Dropout", _C0 + 'layer { name: "drop" type: "Dropout" bottom: "c0" top: "d" dropout_param { dropout_ratio: 0.4 } }\n' + fc("fa", "d") + _S +
        tail(["fa", "fs"]), r"dropout backward into an already written gradient \(drop\)"),
    "Eltwise PROD into an already written gradient": (
        "Eltwise", _C0 + conv("m", "data", 6, "kernel_size: 3 pad: 1", FROZEN) + _ELT % ("m", "PROD") + fc("fa", "t") + _S + tail(["fa", "fs"]),
        r"Eltwise backward into an already written gradient \(t\)"),
    "Eltwise PROD with respect to both bottoms": (
        "Eltwise", _C0 + _O + _ELT % ("o", "PROD") + fc("fa", "t") + _ONE, r"Eltwise PROD backward w.r.t. both bottoms \(t\)"),
    "Eltwise SUM with coefficients": (
        "Eltwise", _C0 + _O + (_ELT % ("o", "SUM")).replace("operation: SUM", "operation: SUM coeff: 1 coeff: -1") + fc("fa", "t") + _ONE,
        r"Eltwise SUM backward with coefficients \(t\)"),
    "a loss whose bottom gradient would accumulate": (
        "SoftmaxWithLoss", _C0 + fc("fa", "c0") + 'layer { name: "loss1" type: "SoftmaxWithLoss" bottom: "fa" bottom: "label" top: "loss1" }\n' +
        fc("fx", "fa") + 'layer { name: "loss2" type: "SoftmaxWithLoss" bottom: "fx" bottom: "label" top: "loss2" }\n',
        r"loss gradient would have to accumulate into fa \(loss1\)"),
    "a learnable depthwise Deconvolution": (
        "Deconvolution", _C0 + (_tconv("up", "kernel_size: 4 stride: 2 pad: 1 bias_term: false", "group: 6") % (6, 'weight_filler { type: "bilinear" }')
                                ).replace("FAN", "c0") + fc("fa", "up") + _ONE, r"learnable depthwise Deconvolution up "),
    "backward through a copied Slice": (
        "Slice", _C0 + 'layer { name: "sl" type: "Slice" bottom: "c0" top: "s0" top: "s1" slice_param { slice_point: 3 } }\n' + fc("fa", "s0") + fc("fs", "s1") +
        tail(["fa", "fs"]), r"backward through the copied Slice sl"),
    "a ReLU with a negative slope below 0": (
        "ReLU", _C0 + _P0 + relu("t", "p0", "t", -0.1) + fc("fa", "t") + _ONE, r"ReLU t: .*negative_slope -0\.1"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("condition", sorted(REFUSALS))
def test_refusals_by_layer_name(gpu, condition):
    """What the planner declines it declines when the engine is built, before any launch, and names the layer."""
    _, text, message = REFUSALS[condition]
    msg, spec = parse(text)
    with pytest.raises(NotImplementedError, match=message):
        TrainEngine(NetSpec(msg, "TRAIN"), dict(spec.input_shapes), device=0, autotune=False)
