"""float64 reference on the CPU for the nets of tests/test_gpu_neuron_fanout.py and tests/test_gpu_neuron_nets.py: a torch interpreter of a
NetSpec with autograd, independent of the engine.  The layers of tests/torch_dw_ref.py and tests/torch_se_ref.py (convolutions with
groups, InnerProduct, BatchNorm with batch or global statistics, Scale with one bottom or - the SE gate - two, Sigmoid, pooling, Eltwise
SUM, Dropout by the device's counter-based mask, the losses) plus the six parameter-free activations, written with torch's own functions:
F.elu, clamp, abs, F.softplus (BNLL) and x * sigmoid(beta x).

masks: {ReLU / ReLU6 / Clip layer: boolean array}, the pass-through masks of ANOTHER forward pass (the device's: y > 0, or lo < y < hi) in
place of the reference's own.  Such a mask is discontinuous: two independently rounded forwards flip it at a handful of activations
next to a bound, which says nothing about the backward kernels.  The forward VALUE stays the reference's own.
cut: layers that pass no gradient to their first bottom (what a backward plan that lost one writer of a shared blob would compute).

Also here, because a test without a GPU reads them too: the fan-out nets (FANOUT) with the layer each of them is about."""
import numpy as np
import torch
import torch.nn.functional as F

from fcn_object_detector_amd.engine import dropout_layer_salt
from fcn_object_detector_amd.netspec import bn_global_stats, kernel_stride_pad, layer_dilation, layer_geometry
from oracle import caffe_ref
from torch_resnet_ref import as_torch, random_params  # noqa: F401  (re-exported for the tests)


def _c(v, x):
    return v.reshape((1, -1) + (1,) * (x.dim() - 2))


def _masked(x, y, mask, dtype):
    """y's value, and a gradient that passes exactly where mask says."""
    m = torch.as_tensor(np.asarray(mask)).reshape(x.shape).to(dtype)
    return y.detach() + (x - x.detach()) * m


def neuron(l, x):
    t = l.type
    if t == "ELU":
        return F.elu(x, alpha=float(l.sub("elu_param").get("alpha", 1.0)))
    if t == "ReLU6":
        return torch.clamp(x, 0.0, 6.0)
    if t == "Clip":
        return torch.clamp(x, float(l.sub("clip_param").get("min")), float(l.sub("clip_param").get("max")))
    if t == "AbsVal":
        return torch.abs(x)
    if t == "BNLL":
        return F.softplus(x, threshold=1e9)
    if t == "Swish":
        return x * torch.sigmoid(float(l.sub("swish_param").get("beta", 1.0)) * x)
    raise NotImplementedError(t)


def clip_bounds(l):
    return (0.0, 6.0) if l.type == "ReLU6" else (float(l.sub("clip_param").get("min")), float(l.sub("clip_param").get("max")))


def torch_net(spec, params, inputs, dtype=torch.float64, dropout_seed=None, updates=None, masks=None, cut=(), round_blob=None):
    """Every blob of the net at its final value; B["total_loss"] = the sum of loss_weight * loss.  updates: a dict that receives
    {BatchNorm layer: [mean sum, variance sum, factor] after this batch-statistics forward}.  round_blob(layer, y) -> y: where a
    half-float engine rounds."""
    B = {k: torch.as_tensor(np.asarray(v, np.float64)).to(dtype) for k, v in inputs.items()}
    total = None
    for l in spec.layers:
        t = l.type
        if t in ("Input", "Python", "Data"):
            continue
        x = B[l.bottoms[0]].detach() if l.name in cut else B[l.bottoms[0]]
        P = params.get(l.name)
        if t in ("Convolution", "DepthwiseConvolution"):
            kh, kw, sh, sw, ph, pw = layer_geometry(l)
            groups = x.shape[1] if t == "DepthwiseConvolution" else int(l.sub("convolution_param").get("group", 1))
            y = F.conv2d(x, P[0], P[1] if len(P) > 1 else None, stride=(sh, sw), padding=(ph, pw), dilation=layer_dilation(l), groups=groups)
        elif t == "InnerProduct":
            y = F.linear(x.reshape(x.shape[0], -1), P[0], P[1] if len(P) > 1 else None)
        elif t in ("ELU", "AbsVal", "BNLL", "Swish"):
            y = neuron(l, x)
        elif t in ("ReLU6", "Clip"):
            y = neuron(l, x)
            if masks is not None and l.name in masks:
                y = _masked(x, y, masks[l.name], dtype)
        elif t == "ReLU":
            y = torch.where(x > 0, x, float(l.sub("relu_param").get("negative_slope", 0.0)) * x)
            if masks is not None and l.name in masks:
                y = _masked(x, y, masks[l.name], dtype)
        elif t == "Sigmoid":
            y = torch.sigmoid(x)
        elif t == "Dropout":
            if spec.phase == "TEST":
                y = x
            else:
                ratio = float(l.sub("dropout_param").get("dropout_ratio", 0.5))
                seed = (dropout_seed + dropout_layer_salt(spec, l)) & 0xFFFFFFFF
                y = x * torch.as_tensor(caffe_ref.dropout_mask(tuple(x.shape), ratio, seed).astype(np.float64)).to(dtype) / (1.0 - ratio)
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
        elif t == "Scale" and len(l.bottoms) == 2:
            g = B[l.bottoms[1]]
            y = x * g.reshape(g.shape[0], g.shape[1], *([1] * (x.dim() - 2)))
        elif t == "Scale":
            y = x * _c(P[0], x) + (_c(P[1], x) if len(P) > 1 else 0.0)
        elif t == "Eltwise":
            assert str(l.sub("eltwise_param").get("operation", "SUM")) == "SUM" and not l.sub("eltwise_param").getall("coeff")
            y = sum(B[b] for b in l.bottoms[1:]) + x
        elif t == "Softmax":
            y = torch.softmax(x, dim=1)
        elif t in ("SoftmaxWithLoss", "EuclideanLoss"):
            if t == "EuclideanLoss":
                y = ((x - B[l.bottoms[1]]) ** 2).sum() / (2.0 * x.shape[0])
            else:
                lab = B[l.bottoms[1]].reshape((x.shape[0],) + tuple(x.shape[2:])).long()
                y = F.cross_entropy(x, lab, reduction="mean")
            wgt = float(l.loss_weight[0]) if l.loss_weight else 1.0
            total = y * wgt if total is None else total + y * wgt
        elif t == "Accuracy":
            y = torch.zeros((), dtype=dtype)      # (a metric: the tests of these nets do not read it)
        else:
            raise NotImplementedError(t)
        assert tuple(y.shape) == tuple(spec.blob_shapes[l.tops[0]]), l.name
        if round_blob is not None:
            y = round_blob(l, y)
        B[l.tops[0]] = y
    if total is not None:
        B["total_loss"] = total
    return B


def device_masks(spec, read_blob):
    """The pass-through masks of the device's forward pass: read_blob(top) of every ReLU (y > 0) and ReLU6 / Clip (lo < y < hi).  Each of
    them is the last layer written in place on its blob in the nets of these tests, so the blob still holds its output."""
    out = {}
    for l in spec.layers:
        if l.type == "ReLU":
            out[l.name] = read_blob(l.tops[0]) > 0
        elif l.type in ("ReLU6", "Clip"):
            lo, hi = clip_bounds(l)
            y = read_blob(l.tops[0])
            out[l.name] = (y > lo) & (y < hi)
    return out


def grad_errors(got, ref, ref32):
    """[(rel_err of the device's gradient, rel_err of torch float32's)] for the blobs of one layer, both against the float64 gradients
    `ref`: max |a - b| over max |b|, the project's measure.  A gradient that is ZERO in exact arithmetic - the bias of a convolution, or
    the beta of a Scale, in front of a BatchNorm with batch statistics, which removes any per-channel shift - comes out of float64
    autograd as rounding noise of 1e-17, and a quotient by that says nothing about either side.  Such a blob (its float64 maximum below
    1e-9 of the largest gradient of the same layer) is measured against that largest gradient instead: the scale of the buffer it
    lies in.  Every other blob keeps its own maximum."""
    refs = [np.asarray(r, np.float64) for r in ref]
    top = max(float(np.abs(r).max()) for r in refs)
    out = []
    for g, r, r32 in zip(got, refs, ref32):
        den = float(np.abs(r).max())
        if den < 1e-9 * top:
            den = top
        den = max(den, 1e-30)
        out.append((float(np.abs(np.asarray(g, np.float64).reshape(r.shape) - r).max()) / den,
                    float(np.abs(np.asarray(r32, np.float64).reshape(r.shape) - r).max()) / den))
    return out


def neuron_params(spec, seed, spread=2.2):
    """tests/torch_resnet_ref.random_params; the biases of SE excite layers (*/se_expand) spread over (-spread, spread) so that the gates
    lie all over (0.1, 0.9), as tests/torch_se_ref.se_params does."""
    params = random_params(spec, seed)
    rng = np.random.default_rng(seed + 1)
    for name, blobs in params.items():
        if name.endswith("/se_expand"):
            blobs[1] = rng.uniform(-spread, spread, blobs[1].shape).astype(np.float32)
    return params


# ---- the fan-out nets of tests/test_gpu_neuron_fanout.py: name -> (prototxt, the layer under test, its type, accumulate) -----------------
_HEAD = """
layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 2 dim: 6 dim: 7 dim: 5 } } }
layer { name: "label" type: "Input" top: "label" input_param { shape { dim: 2 } } }
layer { name: "x" type: "Convolution" bottom: "data" top: "x" convolution_param { num_output: 10 kernel_size: 3 pad: 1 } }
"""
_TAIL = """
layer { name: "feat" type: "Pooling" bottom: "%s" top: "feat" pooling_param { pool: AVE global_pooling: true } }
layer { name: "fc" type: "InnerProduct" bottom: "feat" top: "fc" inner_product_param { num_output: 5 } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc" bottom: "label" top: "loss" }
"""
BODY = {"ELU": 'elu_param { alpha: 0.7 }', "ReLU6": "", "Clip": "clip_param { min: -0.4 max: 0.9 }", "AbsVal": "", "BNLL": "",
        "Swish": "swish_param { beta: 1.4 }"}


def _act(t, bottom="x", top="y"):
    return 'layer { name: "act" type: "%s" bottom: "%s" top: "%s" %s }' % (t, bottom, top, BODY[t])


_OTHER = 'layer { name: "other" type: "Convolution" bottom: "x" top: "z" convolution_param { num_output: 10 kernel_size: 1 } }'
_SUM = 'layer { name: "sum" type: "Eltwise" bottom: "y" bottom: "z" top: "sum" }'
_CONV2 = 'layer { name: "conv2" type: "Convolution" bottom: "x" top: "c2" convolution_param { num_output: 8 kernel_size: 3 pad: 1 } }'
_BN = ('layer { name: "bn" type: "BatchNorm" bottom: "x" top: "x" }\n'
       'layer { name: "sc" type: "Scale" bottom: "x" top: "x" scale_param { bias_term: true } }\n')
_IP = 'layer { name: "ip" type: "InnerProduct" bottom: "x" top: "ip" inner_product_param { num_output: 12 } }\n'
_IP_TAIL = ('layer { name: "fc" type: "InnerProduct" bottom: "ip" top: "fc" inner_product_param { num_output: 5 } }\n'
            'layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc" bottom: "label" top: "loss" }\n')

FANOUT = {}
for _t in BODY:
    # x has two readers.  Backward walks the layers in reverse: the reader written LAST in the file writes G[x] first.
    FANOUT["%s_accumulates" % _t.lower()] = (_HEAD + "\n".join([_act(_t), _OTHER, _SUM]) + _TAIL % "sum", "act", _t, 1)
    FANOUT["%s_writes_first" % _t.lower()] = (_HEAD + "\n".join([_OTHER, _act(_t), _SUM]) + _TAIL % "sum", "act", _t, 0)
for _t in ("ELU", "ReLU6", "Swish"):
    FANOUT["%s_in_place_behind_a_convolution" % _t.lower()] = (_HEAD + _act(_t, "x", "x") + "\n" + _CONV2 + _TAIL % "c2", "act", _t, 0)
    FANOUT["%s_in_place_behind_batchnorm_scale" % _t.lower()] = (_HEAD + _BN + _act(_t, "x", "x") + "\n" + _CONV2 + _TAIL % "c2", "act", _t, 0)
    FANOUT["%s_in_place_behind_an_inner_product" % _t.lower()] = (_HEAD + _IP + _act(_t, "ip", "ip") + "\n" + _IP_TAIL, "act", _t, 0)
for _t in ("Clip", "BNLL"):
    FANOUT["%s_in_place" % _t.lower()] = (_HEAD + _act(_t, "x", "x") + "\n" + _CONV2 + _TAIL % "c2", "act", _t, 0)


def fanout_case(name, seed=51):
    """(NetSpec after infer(), parameters, inputs) of one fan-out net - a bare NetSpec: these layers need no keyword."""
    from fcn_object_detector_amd import proto
    from fcn_object_detector_amd.netspec import NetSpec
    spec = NetSpec(proto.parse_text(FANOUT[name][0]), "TRAIN")
    spec.infer()
    params = random_params(spec, seed)
    rng = np.random.default_rng(seed + 1)
    x = {"data": rng.standard_normal(spec.input_shapes["data"]).astype(np.float32), "label": rng.integers(0, 5, (2,)).astype(np.float32)}
    return spec, params, x
