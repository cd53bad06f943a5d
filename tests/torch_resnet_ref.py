"""float64 reference on the CPU for nets with BatchNorm and Scale (the ResNets): tests/torch_classifier_ref.py's layers plus Caffe's
BatchNormLayer - batch statistics (TRAIN default) or the three blobs' global statistics, and the moving-average step a
batch-statistics forward makes, returned in `updates` - and ScaleLayer over the channel axis.  Blobs written in place are overwritten
in the dictionary, as in the net.  `dtype` float32 runs the same graph in single precision: the reference's own rounding error."""
import numpy as np
import torch
import torch.nn.functional as F

from fcn_object_detector_amd.netspec import bn_global_stats, kernel_stride_pad


def _c(v, x):
    return v.reshape((1, -1) + (1,) * (x.dim() - 2))


def torch_net(spec, params, inputs, round_blob=None, updates=None, dtype=torch.float64, keep=(), relu_masks=None):
    """Every blob of the net (the final value of a blob written in place); B["total_loss"] = sum of loss_weight * loss.  updates: a dict
    that receives {BatchNorm layer: [mean sum, variance sum, factor] after this forward}.  keep: blob names whose tensors retain_grad().
    relu_masks: {ReLU layer: boolean array}, the mask of ANOTHER forward pass (the device's) in place of x > 0 - a ReLU mask is
    discontinuous, two independently rounded forwards flip a handful of near-zero activations, and a flipped mask says nothing about the
    backward kernels (tests/gpu_util.adopt_device_activations is the same step for the CPU oracle)."""
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
            y = F.conv2d(x, P[0], P[1] if len(P) > 1 else None, stride=s, padding=pad, groups=int(p.get("group", 1)))
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
            if str(pp.get("pool", "MAX")) == "MAX":
                y = F.max_pool2d(x, k, s, pad, ceil_mode=True)
            else:
                y = F.avg_pool2d(x, k, s, pad, ceil_mode=True, count_include_pad=True)
            assert tuple(y.shape) == tuple(spec.blob_shapes[l.tops[0]]), l.name
        elif t == "Eltwise":
            assert str(l.sub("eltwise_param").get("operation", "SUM")) == "SUM"
            y = sum(B[b] for b in l.bottoms[1:]) + x
        elif t == "Softmax":
            y = torch.softmax(x, dim=1)
        elif t == "SoftmaxWithLoss":
            y = F.cross_entropy(x, B[l.bottoms[1]].reshape(-1).long(), reduction="mean")
            wgt = float(l.loss_weight[0]) if l.loss_weight else 1.0
            total = y * wgt if total is None else total + y * wgt
        elif t == "Accuracy":
            lab = B[l.bottoms[1]].reshape(-1).long()
            y = ((x > x.gather(1, lab[:, None])).sum(dim=1) < int(l.sub("accuracy_param").get("top_k", 1))).to(dtype).mean()
        else:
            raise NotImplementedError(t)
        if round_blob is not None:
            y = round_blob(l.tops[0], y)
        if l.tops[0] in keep and y.requires_grad:
            y.retain_grad()
        B[l.tops[0]] = y
    if total is not None:
        B["total_loss"] = total
    return B


def as_torch(params, grad=False, dtype=torch.float64):
    return {k: [torch.tensor(np.asarray(a, np.float64), requires_grad=grad and spec_learns(k, i, v), dtype=dtype) for i, a in enumerate(v)]
            for k, v in params.items()}


def spec_learns(name, index, blobs):
    """BatchNorm's three blobs (two vectors and a (1,) factor) are statistics: never leaves of the autograd graph."""
    return not (len(blobs) == 3 and np.asarray(blobs[2]).shape == (1,))


def random_params(spec, seed, factor=2.5):
    """He-scaled convolution and fc banks, small biases; gamma about 0.7 and beta about 0; BatchNorm blobs that are NOT the fillers' zeros:
    mean and variance sums of a non-trivial moving average and a factor that is not 1."""
    rng = np.random.default_rng(seed)
    out = {}
    for l in spec.param_layers():
        shapes = spec.param_shapes[l.name]
        if l.type == "BatchNorm":
            c = shapes[0][0]
            out[l.name] = [(0.3 * rng.standard_normal(c) * factor).astype(np.float32), ((0.5 + rng.random(c)) * factor).astype(np.float32),
                           np.array([factor], np.float32)]
        elif l.type == "Scale":
            out[l.name] = [(0.7 + 0.1 * rng.standard_normal(shapes[0])).astype(np.float32)] + \
                          [(0.1 * rng.standard_normal(s)).astype(np.float32) for s in shapes[1:]]
        else:
            fan_in = int(np.prod(shapes[0][1:]))
            out[l.name] = [(rng.standard_normal(shapes[0]) * np.sqrt(2.0 / fan_in)).astype(np.float32)] + \
                          [(rng.standard_normal(s) * 0.1 + 0.05).astype(np.float32) for s in shapes[1:]]
    return out
