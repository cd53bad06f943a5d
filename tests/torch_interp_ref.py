"""float64 reference on the CPU for nets with Interp layers: tests/torch_dilated_ref.py's layers plus Interp and Concat, as one loop
of its own (that module's loop cannot be entered per layer).  Interp is the pair of weight matrices of tests/ref_interp64.py applied by
einsum: differentiable, and exact where an output falls on an input pixel (a label of 255 stays 255).  `dtype` float32 runs the same
graph in single precision: the reference's own rounding error.  relu_masks / pool_argmax as in tests/torch_dilated_ref.py."""
import numpy as np
import torch
import torch.nn.functional as F

import ref_interp64 as R
from fcn_object_detector_amd.engine import dropout_layer_salt
from fcn_object_detector_amd.netspec import interp_size, kernel_stride_pad, layer_dilation
from oracle import caffe_ref as C
from torch_dilated_ref import as_torch, max_pool_argmax, random_params  # noqa: F401  (re-exported for the tests)


def interp(x, l):
    h, w = x.shape[2:]
    oh, ow, pb, pe = interp_size(l, h, w)
    off, he, we = R.window(h, w, pb, pe)
    wy, wx = (torch.as_tensor(R.weights(n1, n2)).to(x.dtype) for n1, n2 in ((he, oh), (we, ow)))
    return torch.einsum("oh,nchw,pw->ncop", wy, x[:, :, off:off + he, off:off + we], wx)


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
                y = x * torch.as_tensor(C.dropout_mask(tuple(x.shape), ratio, seed).astype(np.float64)).to(dtype) / (1.0 - ratio)
        elif t == "Interp":
            y = interp(x, l)
        elif t == "Concat":
            y = torch.cat([B[b] for b in l.bottoms], dim=1)
        elif t == "SoftmaxWithLoss":
            ign = l.sub("loss_param").get("ignore_label")
            lab = B[l.bottoms[1]][:, 0].long()
            y = F.cross_entropy(x, lab, ignore_index=int(ign) if ign is not None else -100, reduction="mean")
            wgt = float(l.loss_weight[0]) if l.loss_weight else 1.0
            total = y * wgt if total is None else total + y * wgt
        else:
            raise NotImplementedError(t)
        assert tuple(y.shape) == tuple(spec.blob_shapes[l.tops[0]]), l.name
        B[l.tops[0]] = y
    if total is not None:
        B["total_loss"] = total
    return B
