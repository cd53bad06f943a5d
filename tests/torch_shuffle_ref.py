"""float64 reference on the CPU for the nets of tests/test_gpu_shuffle_fanout.py and tests/test_gpu_shuffle_nets.py: a torch interpreter of a
NetSpec with autograd, independent of the engine.  The layers of a ShuffleNet - convolutions with groups (depthwise in either
spelling), InnerProduct, BatchNorm with batch or global statistics, Scale, ReLU, MAX and AVE pooling by Caffe's shape rule, Eltwise SUM,
Concat, Slice, Softmax and the loss - and ShuffleChannel as `reshape -> transpose -> reshape`, which is not how tests/ref_shuffle64.py or
the kernel index it.

masks: {ReLU layer: boolean array}, the pass-through masks of ANOTHER forward pass (the device's) in place of the reference's own - two
independently rounded forwards flip such a mask at a handful of activations next to 0, which says nothing about the backward kernels.
The forward VALUE stays the reference's own.
cut: layers that pass no gradient to their first bottom (what a backward plan that lost one writer of a shared blob would compute).

Also here, because a test without a GPU reads them too: the fan-out nets (FANOUT) with the layer each of them is about."""
import numpy as np
import torch
import torch.nn.functional as F

from fcn_object_detector_amd.netspec import bn_global_stats, kernel_stride_pad, layer_dilation, layer_geometry
from torch_neuron_ref import grad_errors  # noqa: F401  (re-exported for the tests)
from torch_resnet_ref import as_torch, random_params  # noqa: F401  (re-exported for the tests)


def _c(v, x):
    return v.reshape((1, -1) + (1,) * (x.dim() - 2))


def shuffle(x, g):
    n, c = x.shape[:2]
    rest = tuple(x.shape[2:])
    return x.reshape((n, g, c // g) + rest).transpose(1, 2).reshape((n, c) + rest)


def torch_net(spec, params, inputs, dtype=torch.float64, updates=None, masks=None, cut=()):
    """Every blob of the net at its final value; B["total_loss"] = the sum of loss_weight * loss.  updates: a dict that receives
    {BatchNorm layer: [mean sum, variance sum, factor] after this batch-statistics forward}."""
    B = {k: torch.as_tensor(np.asarray(v, np.float64)).to(dtype) for k, v in inputs.items()}
    total = None
    for l in spec.layers:
        t = l.type
        if t in ("Input", "Python", "Data"):
            continue
        x = B[l.bottoms[0]].detach() if l.name in cut else B[l.bottoms[0]]
        P = params.get(l.name)
        if t == "Slice":
            pts = [int(v) for v in l.sub("slice_param").getall("slice_point")]
            edges = [0] + pts + [x.shape[1]]
            for tp, a, b in zip(l.tops, edges[:-1], edges[1:]):
                B[tp] = x[:, a:b]
                assert tuple(B[tp].shape) == tuple(spec.blob_shapes[tp]), l.name
            continue
        if t in ("Convolution", "DepthwiseConvolution"):
            kh, kw, sh, sw, ph, pw = layer_geometry(l)
            groups = x.shape[1] if t == "DepthwiseConvolution" else int(l.sub("convolution_param").get("group", 1))
            y = F.conv2d(x, P[0], P[1] if len(P) > 1 else None, stride=(sh, sw), padding=(ph, pw), dilation=layer_dilation(l), groups=groups)
        elif t == "InnerProduct":
            y = F.linear(x.reshape(x.shape[0], -1), P[0], P[1] if len(P) > 1 else None)
        elif t == "ShuffleChannel":
            y = shuffle(x, int(l.sub("shuffle_channel_param").get("group", 1)))
        elif t == "ReLU":
            y = torch.relu(x)
            if masks is not None and l.name in masks:
                m = torch.as_tensor(np.asarray(masks[l.name])).reshape(x.shape).to(dtype)
                y = y.detach() + (x - x.detach()) * m
        elif t == "Pooling":
            pp = l.sub("pooling_param")
            k, s, pad = (tuple(x.shape[2:]), 1, 0) if bool(pp.get("global_pooling", False)) else kernel_stride_pad(pp)
            if str(pp.get("pool", "MAX")) == "MAX":
                y = F.max_pool2d(x, k, s, pad, ceil_mode=True)
            else:
                y = F.avg_pool2d(x, k, s, pad, ceil_mode=True, count_include_pad=True)
        elif t == "BatchNorm":
            bp = l.sub("batch_norm_param")
            eps = float(bp.get("eps", 1e-5))
            dims = [d for d in range(x.dim()) if d != 1]
            if bn_global_stats(l, spec.phase):
                fac = float(P[2].reshape(-1)[0])
                sc = 0.0 if fac == 0.0 else 1.0 / fac
                mean, var = (sc * P[0]).detach(), (sc * P[1]).detach()
            else:
                mean = x.mean(dim=dims)
                var = ((x - _c(mean, x)) ** 2).mean(dim=dims)
                if updates is not None:
                    m, f = x.numel() // x.shape[1], float(bp.get("moving_average_fraction", 0.999))
                    updates[l.name] = [(P[0] * f + mean).detach().double().numpy(),
                                       (P[1] * f + var * (m / (m - 1.0) if m > 1 else 1.0)).detach().double().numpy(),
                                       (P[2] * f + 1.0).detach().double().numpy()]
            y = (x - _c(mean, x)) / torch.sqrt(_c(var, x) + eps)
        elif t == "Scale":
            y = x * _c(P[0], x) + (_c(P[1], x) if len(P) > 1 else 0.0)
        elif t == "Eltwise":
            assert str(l.sub("eltwise_param").get("operation", "SUM")) == "SUM" and not l.sub("eltwise_param").getall("coeff")
            y = sum(B[b] for b in l.bottoms[1:]) + x
        elif t == "Concat":
            y = torch.cat([x] + [B[b] for b in l.bottoms[1:]], dim=1)
        elif t == "Softmax":
            y = torch.softmax(x, dim=1)
        elif t == "SoftmaxWithLoss":
            lab = B[l.bottoms[1]].reshape((x.shape[0],) + tuple(x.shape[2:])).long()
            y = F.cross_entropy(x, lab, reduction="mean")
            wgt = float(l.loss_weight[0]) if l.loss_weight else 1.0
            total = y * wgt if total is None else total + y * wgt
        elif t == "Accuracy":
            y = torch.zeros((), dtype=dtype)      # (a metric: the tests of these nets do not read it)
        else:
            raise NotImplementedError(t)
        assert tuple(y.shape) == tuple(spec.blob_shapes[l.tops[0]]), l.name
        B[l.tops[0]] = y
    if total is not None:
        B["total_loss"] = total
    return B


def device_masks(spec, read_blob):
    """The pass-through masks of the device's forward pass: read_blob(top) > 0 of every ReLU.  Each of them is the last layer written in
    place on its blob in the nets of these tests, so the blob still holds its output."""
    return {l.name: read_blob(l.tops[0]) > 0 for l in spec.layers if l.type == "ReLU"}


# ---- the fan-out nets of tests/test_gpu_shuffle_fanout.py: name -> (prototxt, the layer under test, its type, accumulate) ----------------
_HEAD = """
layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 2 dim: 8 dim: 7 dim: 5 } } }
layer { name: "label" type: "Input" top: "label" input_param { shape { dim: 2 } } }
"""
_TAIL = """
layer { name: "feat" type: "Pooling" bottom: "%s" top: "feat" pooling_param { pool: AVE global_pooling: true } }
layer { name: "fc" type: "InnerProduct" bottom: "feat" top: "fc" inner_product_param { num_output: 5 } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc" bottom: "label" top: "loss" }
"""


def _conv(name, bottom, top, n, k=1, group=1):
    return ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: %d kernel_size: %d pad: %d group: %d } }'
            % (name, bottom, top, n, k, k // 2, group))


def _sh(bottom, top="y", group=2):
    return 'layer { name: "sh" type: "ShuffleChannel" bottom: "%s" top: "%s" shuffle_channel_param { group: %d } }' % (bottom, top, group)


_GROUPED = _conv("x", "data", "x", 16, 3, 2)                         # 4 input and 8 output channels per group
_BRANCHES = "\n".join([_conv("a", "data", "a", 8, 3), _conv("b", "data", "b", 8, 1),
                       'layer { name: "x" type: "Concat" bottom: "a" bottom: "b" top: "x" }'])
_SUM = 'layer { name: "sum" type: "Eltwise" bottom: "%s" bottom: "z" top: "sum" }'
_OTHER = _conv("other", "x", "z", 16)
_SLICED = "\n".join(['layer { name: "sl" type: "Slice" bottom: "y" top: "l" top: "r" slice_param { axis: 1 slice_point: 8 } }',
                     _conv("right", "r", "r2", 8, 3), 'layer { name: "cat" type: "Concat" bottom: "l" bottom: "r2" top: "cat" }'])

FANOUT = {}
for _name, _front in (("behind_a_grouped_convolution", _GROUPED), ("behind_a_concat_of_two_branches", _BRANCHES)):
    # x has two readers.  Backward walks the layers in reverse: the reader written LAST in the file writes G[x] first.
    FANOUT[_name + "_accumulates"] = (_HEAD + "\n".join([_front, _sh("x"), _OTHER, _SUM % "y"]) + _TAIL % "sum", "sh", "ShuffleChannel", 1)
    FANOUT[_name + "_writes_first"] = (_HEAD + "\n".join([_front, _OTHER, _sh("x"), _SUM % "y"]) + _TAIL % "sum", "sh", "ShuffleChannel", 0)
FANOUT["in_front_of_a_slice_accumulates"] = (_HEAD + "\n".join([_GROUPED, _sh("x"), _SLICED, _OTHER, _SUM % "cat"]) + _TAIL % "sum",
                                             "sh", "ShuffleChannel", 1)
FANOUT["in_front_of_a_slice_alone"] = (_HEAD + "\n".join([_GROUPED, _sh("x"), _SLICED]) + _TAIL % "cat", "sh", "ShuffleChannel", 0)
FANOUT["on_a_2d_blob"] = (_HEAD + 'layer { name: "x" type: "InnerProduct" bottom: "data" top: "x" inner_product_param { num_output: 12 } }\n'
                          + _sh("x", group=3) + '\nlayer { name: "fc" type: "InnerProduct" bottom: "y" top: "fc" inner_product_param { num_output: 5 } }\n'
                          'layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc" bottom: "label" top: "loss" }\n', "sh", "ShuffleChannel", 0)


def fanout_case(name, seed=61):
    """(NetSpec after infer(), parameters, inputs) of one fan-out net - a bare NetSpec: the layer needs no keyword."""
    from fcn_object_detector_amd import proto
    from fcn_object_detector_amd.netspec import NetSpec
    spec = NetSpec(proto.parse_text(FANOUT[name][0]), "TRAIN")
    spec.infer()
    params = random_params(spec, seed)
    rng = np.random.default_rng(seed + 1)
    x = {"data": rng.standard_normal(spec.input_shapes["data"]).astype(np.float32), "label": rng.integers(0, 5, (2,)).astype(np.float32)}
    return spec, params, x
