"""float64 reference on the CPU for nets with rectangular convolutions (Inception-v3, factorised residual blocks): torch's conv2d with
the per-axis stride / padding of netspec.layer_geometry and the layer's dilation, plus what tests/torch_resnet_ref.py and
tests/torch_dilated_ref.py have - Caffe's BatchNormLayer (batch or global statistics) and ScaleLayer over the channel axis, Concat,
MAX / AVE pooling in Caffe's ceil mode and global pooling, InnerProduct, the device's counter-based Dropout mask, Eltwise SUM, Softmax,
SoftmaxWithLoss and Accuracy over an (N,) label, EuclideanLoss.  Blobs written in place are overwritten in the dictionary, as in the
net.  `dtype` float32 runs the same graph in single precision: the reference's own rounding error.  relu_masks: {ReLU layer: boolean
array} and pool_argmax: {MAX Pooling layer: index tensor} are the masks and argmaxes of ANOTHER forward pass (the device's) in place of
the reference's own, as the two files above explain: both are discontinuous, and a flipped unit says nothing about a backward kernel."""
import numpy as np
import torch
import torch.nn.functional as F

from fcn_object_detector_amd.engine import dropout_layer_salt
from fcn_object_detector_amd.netspec import bn_global_stats, kernel_stride_pad, layer_dilation, layer_geometry
from oracle import caffe_ref as R
from torch_resnet_ref import as_torch, random_params      # noqa: F401  (BatchNorm blobs are never leaves; He-scaled banks)


def _c(v, x):
    return v.reshape((1, -1) + (1,) * (x.dim() - 2))


def torch_net(spec, params, inputs, dropout_seed=None, dtype=torch.float64, relu_masks=None, pool_argmax=None, updates=None):
    """Every blob of the net; B["total_loss"] = sum of loss_weight * loss.  updates receives {BatchNorm layer: its three blobs after a
    batch-statistics forward}."""
    B = {k: torch.as_tensor(np.asarray(v, np.float64)).to(dtype) for k, v in inputs.items()}
    total = None
    for l in spec.layers:
        t = l.type
        if t in ("Input", "Python", "Data"):
            continue
        x = B[l.bottoms[0]]
        P = params.get(l.name)
        if t == "Convolution":
            kh, kw, sh, sw, ph, pw = layer_geometry(l)
            assert tuple(P[0].shape[2:]) == (kh, kw), l.name
            y = F.conv2d(x, P[0], P[1] if len(P) > 1 else None, stride=(sh, sw), padding=(ph, pw), dilation=layer_dilation(l),
                         groups=int(l.sub("convolution_param").get("group", 1)))
            assert tuple(y.shape) == tuple(spec.blob_shapes[l.tops[0]]), l.name
        elif t == "InnerProduct":
            y = F.linear(x.reshape(x.shape[0], -1), P[0], P[1] if len(P) > 1 else None)
        elif t == "BatchNorm":
            bp = l.sub("batch_norm_param")
            eps, f = float(bp.get("eps", 1e-5)), float(bp.get("moving_average_fraction", 0.999))
            dims = [d for d in range(x.dim()) if d != 1]
            if bn_global_stats(l, spec.phase):
                fac = float(P[2].reshape(-1)[0])
                sc = 0.0 if fac == 0.0 else 1.0 / fac
                mean, var = (sc * P[0]).detach(), (sc * P[1]).detach()
            else:
                mean = x.mean(dim=dims)
                var = ((x - _c(mean, x)) ** 2).mean(dim=dims)
                m = x.numel() // x.shape[1]
                if updates is not None:
                    corr = m / (m - 1.0) if m > 1 else 1.0
                    updates[l.name] = [(P[0] * f + mean).detach().double().numpy(), (P[1] * f + var * corr).detach().double().numpy(),
                                       (P[2] * f + 1.0).detach().double().numpy()]
            y = (x - _c(mean, x)) / torch.sqrt(_c(var, x) + eps)
        elif t == "Scale":
            y = x * _c(P[0], x)
            if len(P) > 1:
                y = y + _c(P[1], x)
        elif t == "ReLU":
            y = torch.relu(x) if relu_masks is None else x * torch.as_tensor(np.asarray(relu_masks[l.name])).to(dtype)
        elif t == "Pooling":
            pp = l.sub("pooling_param")
            k, s, pad = (tuple(x.shape[2:]), 1, 0) if bool(pp.get("global_pooling", False)) else kernel_stride_pad(pp)
            if str(pp.get("pool", "MAX")) == "MAX" and pool_argmax is not None:
                idx = pool_argmax[l.name]
                y = x.flatten(2).gather(2, idx.flatten(2)).reshape(idx.shape)
            elif str(pp.get("pool", "MAX")) == "MAX":
                y = F.max_pool2d(x, k, s, pad, ceil_mode=True)
            else:
                y = F.avg_pool2d(x, k, s, pad, ceil_mode=True, count_include_pad=True)
            assert tuple(y.shape) == tuple(spec.blob_shapes[l.tops[0]]), l.name
        elif t == "Concat":
            y = torch.cat([B[b] for b in l.bottoms], dim=1)
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
        elif t == "Softmax":
            y = torch.softmax(x, dim=1)
        elif t in ("SoftmaxWithLoss", "EuclideanLoss"):
            if t == "SoftmaxWithLoss":
                y = F.cross_entropy(x, B[l.bottoms[1]].reshape(-1).long(), reduction="mean")
            else:
                y = ((x - B[l.bottoms[1]]) ** 2).sum() / (2.0 * x.shape[0])
            wgt = float(l.loss_weight[0]) if l.loss_weight else 1.0
            total = y * wgt if total is None else total + y * wgt
        elif t == "Accuracy":
            lab = B[l.bottoms[1]].reshape(-1).long()
            y = ((x > x.gather(1, lab[:, None])).sum(dim=1) < int(l.sub("accuracy_param").get("top_k", 1))).to(dtype).mean()
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
        if l.type == "Pooling" and str(pp.get("pool", "MAX")) == "MAX" and not bool(pp.get("global_pooling", False)):
            k, s, pad = kernel_stride_pad(pp)
            out[l.name] = F.max_pool2d(torch.as_tensor(np.asarray(read_blob(l.bottoms[0]), np.float64)), k, s, pad, ceil_mode=True, return_indices=True)[1]
    return out
