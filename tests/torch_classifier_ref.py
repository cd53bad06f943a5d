"""float64 reference on the CPU for the classifier-style nets (CaffeNet, GOTURN, BVLC GoogLeNet): tests/test_gpu_fcn_published.py's
torch_net with what those nets add - grouped conv2d, InnerProduct as `linear` over the (c, h, w)-flattened input, AVE pooling
(avg_pool2d, ceil mode, the padding counted in the divisor), LRN, Concat, Eltwise SUM, L1Loss, SoftmaxWithLoss over (N, C) scores with (N,) labels
and loss weights, Accuracy.  `round_blob(name, tensor)`, when given, is applied to every blob as it is stored: the half-float engine's
rounding points."""
import numpy as np
import torch
import torch.nn.functional as F

from fcn_object_detector_amd.engine import dropout_layer_salt
from fcn_object_detector_amd.netspec import kernel_stride_pad
from oracle import caffe_ref as R


def torch_net(spec, params, inputs, dropout_seed=None, round_blob=None):
    """Every blob of the net; B["total_loss"] = sum of loss_weight * loss over the loss layers (what the solver minimises)."""
    B = {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in inputs.items()}
    total = None
    for l in spec.layers:
        t = l.type
        if t in ("Input", "Python", "Data"):
            continue
        x = B[l.bottoms[0]]
        if t == "Convolution":
            p = l.sub("convolution_param")
            k, s, pad = kernel_stride_pad(p)
            w, b = params[l.name][0], (params[l.name][1] if len(params[l.name]) > 1 else None)
            y = F.conv2d(x, w, b, stride=s, padding=pad, groups=int(p.get("group", 1)))
        elif t == "InnerProduct":
            w, b = params[l.name][0], (params[l.name][1] if len(params[l.name]) > 1 else None)
            y = F.linear(x.reshape(x.shape[0], -1), w, b)
        elif t == "ReLU":
            y = torch.relu(x)
        elif t == "Pooling":
            pp = l.sub("pooling_param")
            if bool(pp.get("global_pooling", False)):
                k, s, pad = x.shape[2], 1, 0
            else:
                k, s, pad = kernel_stride_pad(pp)
            if str(pp.get("pool", "MAX")) == "MAX":
                y = F.max_pool2d(x, k, s, pad, ceil_mode=True)
            else:
                y = F.avg_pool2d(x, k, s, pad, ceil_mode=True, count_include_pad=True)
            assert tuple(y.shape) == tuple(spec.blob_shapes[l.tops[0]]), l.name
        elif t == "LRN":
            p = l.sub("lrn_param")
            y = F.local_response_norm(x, int(p.get("local_size", 5)), float(p.get("alpha", 1.0)), float(p.get("beta", 0.75)), float(p.get("k", 1.0)))
        elif t == "Eltwise":
            assert str(l.sub("eltwise_param").get("operation", "SUM")) == "SUM"
            y = sum(B[b] for b in l.bottoms[1:]) + x
        elif t == "Concat":
            y = torch.cat([B[b] for b in l.bottoms], dim=1)
        elif t == "Dropout":
            if spec.phase == "TEST":
                y = x
            else:
                ratio = float(l.sub("dropout_param").get("dropout_ratio", 0.5))
                seed = (dropout_seed + dropout_layer_salt(spec, l)) & 0xFFFFFFFF
                y = x * torch.as_tensor(R.dropout_mask(tuple(x.shape), ratio, seed).astype(np.float64)) / (1.0 - ratio)
        elif t == "Softmax":
            y = torch.softmax(x, dim=1)
        elif t in ("SoftmaxWithLoss", "L1Loss"):
            if t == "L1Loss":
                y = (x - B[l.bottoms[1]]).abs().sum() / x.shape[0]
            else:
                y = F.cross_entropy(x, B[l.bottoms[1]].reshape(-1).long(), reduction="mean")
            wgt = float(l.loss_weight[0]) if l.loss_weight else 1.0
            total = y * wgt if total is None else total + y * wgt
        elif t == "Accuracy":
            top_k = int(l.sub("accuracy_param").get("top_k", 1))
            lab = B[l.bottoms[1]].reshape(-1).long()
            picked = x.gather(1, lab[:, None])
            y = ((x > picked).sum(dim=1) < top_k).double().mean()      # the label's score is among the top_k largest
        else:
            raise NotImplementedError(t)
        if round_blob is not None:
            y = round_blob(l.tops[0], y)
        B[l.tops[0]] = y
    if total is not None:
        B["total_loss"] = total
    return B


def as_torch(params, grad=False):
    return {k: [torch.tensor(np.asarray(a, np.float64), requires_grad=grad) for a in v] for k, v in params.items()}


def random_params(spec, seed):
    """He-scaled normal weights and small random biases: the published fillers (gaussian 0.01, constant biases) leave a width-reduced
    net with vanishing activations and every bias of a layer equal."""
    rng = np.random.default_rng(seed)
    out = {}
    for l in spec.param_layers():
        shapes = spec.param_shapes[l.name]
        fan_in = int(np.prod(shapes[0][1:]))
        blobs = [(rng.standard_normal(shapes[0]) * np.sqrt(2.0 / fan_in)).astype(np.float32)]
        if len(shapes) > 1:
            blobs.append((rng.standard_normal(shapes[1]) * 0.1 + 0.05).astype(np.float32))
        out[l.name] = blobs
    return out
