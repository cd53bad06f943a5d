"""float64 reference on the CPU for the dilated nets (DeepLab-LargeFOV, the DeepLab-v2 ASPP head): torch's conv2d(..., dilation=d),
max_pool2d / avg_pool2d in Caffe's ceil mode, the device's counter-based Dropout mask, Eltwise SUM, SoftmaxWithLoss and Accuracy with
an ignore_label over a 4-d score map.  Blobs written in place are overwritten in the dictionary, as in the net.  `dtype` float32 runs
the same graph in single precision: the reference's own rounding error.  relu_masks: {ReLU layer: boolean array}, the mask of ANOTHER
forward pass (the device's) in place of x > 0, as tests/torch_resnet_ref.py explains.  pool_argmax: {MAX Pooling layer: index tensor},
the argmaxes of that other forward pass in place of the reference's own - the same discontinuity: these nets pool 3x3 windows at
stride 1 over ReLU outputs, and where a window is all zeros but for one unit that one pass rounds to +1e-9 and the other to -1e-9,
the window's whole gradient goes to that unit in one pass and nowhere in the other (tests/gpu_util.adopt_device_activations takes
the device's argmaxes for the CPU oracle for the same reason)."""
import numpy as np
import torch
import torch.nn.functional as F

from fcn_object_detector_amd.engine import dropout_layer_salt
from fcn_object_detector_amd.netspec import kernel_stride_pad, layer_dilation
from oracle import caffe_ref as R


def torch_net(spec, params, inputs, dropout_seed=None, dtype=torch.float64, relu_masks=None, pool_argmax=None):
    """Every blob of the net; B["total_loss"] = sum of loss_weight * loss."""
    B = {k: torch.as_tensor(np.asarray(v, np.float64)).to(dtype) for k, v in inputs.items()}
    total = None
    for l in spec.layers:
        t = l.type
        if t in ("Input", "Python", "Data"):
            continue
        x = B[l.bottoms[0]]
        P = params.get(l.name)
        if t == "Convolution":
            p = l.sub("convolution_param")
            k, s, pad = kernel_stride_pad(p)
            y = F.conv2d(x, P[0], P[1] if len(P) > 1 else None, stride=s, padding=pad, dilation=layer_dilation(l), groups=int(p.get("group", 1)))
        elif t == "ReLU":
            y = torch.relu(x) if relu_masks is None else x * torch.as_tensor(np.asarray(relu_masks[l.name])).to(dtype)
        elif t == "Pooling":
            pp = l.sub("pooling_param")
            k, s, pad = kernel_stride_pad(pp)
            if str(pp.get("pool", "MAX")) == "MAX" and pool_argmax is not None:
                idx = pool_argmax[l.name]
                y = x.flatten(2).gather(2, idx.flatten(2)).reshape(idx.shape)
            elif str(pp.get("pool", "MAX")) == "MAX":
                y = F.max_pool2d(x, k, s, pad, ceil_mode=True)
            else:
                y = F.avg_pool2d(x, k, s, pad, ceil_mode=True, count_include_pad=True)
            assert tuple(y.shape) == tuple(spec.blob_shapes[l.tops[0]]), l.name
        elif t == "Dropout":
            if spec.phase == "TEST":
                y = x
            else:
                ratio = float(l.sub("dropout_param").get("dropout_ratio", 0.5))
                seed = (dropout_seed + dropout_layer_salt(spec, l)) & 0xFFFFFFFF
                y = x * torch.as_tensor(R.dropout_mask(tuple(x.shape), ratio, seed).astype(np.float64)).to(dtype) / (1.0 - ratio)
        elif t == "Eltwise":
            assert str(l.sub("eltwise_param").get("operation", "SUM")) == "SUM"
            y = sum(B[b] for b in l.bottoms[1:]) + x
        elif t == "SoftmaxWithLoss":
            ign = l.sub("loss_param").get("ignore_label")
            lab = B[l.bottoms[1]][:, 0].long()
            y = F.cross_entropy(x, lab, ignore_index=int(ign) if ign is not None else -100, reduction="mean")
            wgt = float(l.loss_weight[0]) if l.loss_weight else 1.0
            total = y * wgt if total is None else total + y * wgt
        elif t == "Accuracy":
            ign = l.sub("accuracy_param").get("ignore_label")
            lab = B[l.bottoms[1]][:, 0].long()
            valid = lab != int(ign) if ign is not None else torch.ones_like(lab, dtype=torch.bool)
            safe = torch.where(valid, lab, torch.zeros_like(lab))
            right = (x >= x.gather(1, safe[:, None])).sum(dim=1) <= 1      # (ties count against the label)
            y = (right & valid).sum().to(dtype) / valid.sum().clamp(min=1).to(dtype)
        else:
            raise NotImplementedError(t)
        B[l.tops[0]] = y
    if total is not None:
        B["total_loss"] = total
    return B


def max_pool_argmax(spec, read_blob):
    """{MAX Pooling layer: argmax indices (iy * W + ix per plane)} of the forward pass whose blobs read_blob(name) returns."""
    out = {}
    for l in spec.layers:
        pp = l.sub("pooling_param")
        if l.type == "Pooling" and str(pp.get("pool", "MAX")) == "MAX":
            k, s, pad = kernel_stride_pad(pp)
            out[l.name] = F.max_pool2d(torch.as_tensor(np.asarray(read_blob(l.bottoms[0]), np.float64)), k, s, pad, ceil_mode=True, return_indices=True)[1]
    return out


def as_torch(params, grad=False, dtype=torch.float64):
    return {k: [torch.tensor(np.asarray(a, np.float64), requires_grad=grad, dtype=dtype) for a in v] for k, v in params.items()}


def random_params(spec, seed):
    """He-scaled banks and small biases: activations of order 1 through every layer, so no blob is a near-zero difference.  The score
    layers (fc8_*) get a quarter of that scale: at He's scale the sum of the four ASPP scores reaches a negative log-likelihood of 88.5
    at one pixel, where Caffe's SoftmaxWithLoss - and the kernel - clamps the probability at FLT_MIN (-log = 87.34) and torch's
    cross_entropy does not: a difference of definitions at an input no trained net produces, not an error of either."""
    rng = np.random.default_rng(seed)
    out = {}
    for l in spec.param_layers():
        shapes = spec.param_shapes[l.name]
        fan_in = int(np.prod(shapes[0][1:])) * (16 if l.name.startswith("fc8") else 1)
        out[l.name] = [(rng.standard_normal(shapes[0]) * np.sqrt(2.0 / fan_in)).astype(np.float32)] + \
                      [(rng.standard_normal(s) * 0.1 + 0.05).astype(np.float32) for s in shapes[1:]]
    return out
