"""float64 reference on the CPU for the encoder-decoder nets (SegNet, SegNet-Basic): tests/torch_resnet_ref.py's Convolution,
BatchNorm and Scale, MAX pooling with its indices (max_pool2d(return_indices=True)) as the mask blob, the Upsample layer as
max_unpool2d by that mask, Softmax, and SoftmaxWithLoss / Accuracy with an ignore_label over a 4-d score map.

torch's pooling and Caffe's share the window rule for 2 x 2 / stride 2 on even extents only (tests/test_unpool_ref.py): this file is a
reference for such nets alone, and says so with an assertion.  Blobs written in place are overwritten in the dictionary, as in the net.
`dtype` float32 runs the same graph in single precision: the reference's own rounding error.  relu_masks: {ReLU layer: boolean array}
and pool_idx: {MAX Pooling layer: index array}, the masks and argmaxes of ANOTHER forward pass (the device's) in place of the
reference's own, for the reasons tests/torch_dilated_ref.py gives - here the argmax also decides where the decoder puts a value."""
import numpy as np
import torch
import torch.nn.functional as F

from fcn_object_detector_amd.netspec import bn_global_stats, kernel_stride_pad
from torch_resnet_ref import as_torch, random_params  # noqa: F401  (re-exported: the tests take them from here)


def _c(v, x):
    return v.reshape((1, -1) + (1,) * (x.dim() - 2))


def torch_net(spec, params, inputs, dtype=torch.float64, relu_masks=None, pool_idx=None):
    """Every blob of the net, the masks as int64 tensors; B["total_loss"] = sum of loss_weight * loss."""
    B = {k: torch.as_tensor(np.asarray(v, np.float64)).to(dtype) for k, v in inputs.items()}
    total = None
    for l in spec.layers:
        t = l.type
        if t in ("Input", "Python", "Data"):
            continue
        x = B[l.bottoms[0]]
        P = params.get(l.name)
        if t == "Convolution":
            k, s, pad = kernel_stride_pad(l.sub("convolution_param"))
            y = F.conv2d(x, P[0], P[1] if len(P) > 1 else None, stride=s, padding=pad)
        elif t == "BatchNorm":
            eps = float(l.sub("batch_norm_param").get("eps", 1e-5))
            dims = [d for d in range(x.dim()) if d != 1]
            if bn_global_stats(l, spec.phase):
                fac = float(P[2].reshape(-1)[0])
                sc = 0.0 if fac == 0.0 else 1.0 / fac
                mean, var = (sc * P[0]).detach(), (sc * P[1]).detach()
            else:
                mean = x.mean(dim=dims)
                var = ((x - _c(mean, x)) ** 2).mean(dim=dims)
            y = (x - _c(mean, x)) / torch.sqrt(_c(var, x) + eps)
        elif t == "Scale":
            y = x * _c(P[0], x)
            if len(P) > 1:
                y = y + _c(P[1], x)
        elif t == "ReLU":
            y = torch.relu(x) if relu_masks is None else x * torch.as_tensor(np.asarray(relu_masks[l.name])).to(dtype)
        elif t == "Pooling":
            k, s, pad = kernel_stride_pad(l.sub("pooling_param"))
            assert (k, s, pad) == (2, 2, 0) and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0, "torch's window rule is Caffe's only here"
            if pool_idx is not None:
                idx = torch.as_tensor(np.asarray(pool_idx[l.name]).astype(np.int64))
                y = x.flatten(2).gather(2, idx.flatten(2)).reshape(idx.shape)
            else:
                y, idx = F.max_pool2d(x, k, s, pad, ceil_mode=True, return_indices=True)
            if len(l.tops) > 1:
                B[l.tops[1]] = idx
        elif t == "Upsample":
            pool = spec.mask_blobs[l.bottoms[1]]
            k, s, pad = kernel_stride_pad(pool.sub("pooling_param"))
            y = F.max_unpool2d(x, B[l.bottoms[1]], k, s, pad, output_size=tuple(spec.blob_shapes[l.tops[0]][2:]))
        elif t == "Softmax":
            y = torch.softmax(x, dim=1)
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
        assert tuple(y.shape) == tuple(spec.blob_shapes[l.tops[0]]), l.name
        B[l.tops[0]] = y
    if total is not None:
        B["total_loss"] = total
    return B
