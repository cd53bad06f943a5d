"""float64 reference on the CPU for the SE-ResNets (models.se_resnet): tests/torch_resnet_ref.py's layers plus Sigmoid and Caffe's ScaleLayer
with two bottoms over axis 0 - y = x * gate[n, c] - which is also what an Axpy layer is once a NetSpec built with scale_gate=True has read
it (a gated Scale and an Eltwise SUM).  Blobs written in place are overwritten in the dictionary, as in the net.  `dtype` float32 runs
the same graph in single precision: the reference's own rounding error."""
import numpy as np
import torch
import torch.nn.functional as F

from fcn_object_detector_amd.netspec import bn_global_stats, kernel_stride_pad
from torch_resnet_ref import _c, as_torch, random_params      # noqa: F401  (re-exported for the tests)


def torch_se_net(spec, params, inputs, round_blob=None, dtype=torch.float64, relu_masks=None, updates=None):
    """Every blob of the net; B["total_loss"] = the sum of the losses.  round_blob(layer, top, y) -> y: where a half-float engine rounds.
    updates: a dict that receives {BatchNorm layer: [mean sum, variance sum, factor] after this batch-statistics forward}.
    relu_masks: {ReLU layer: boolean array}, the masks of another forward pass (tests/torch_resnet_ref.py says why)."""
    B = {k: torch.as_tensor(np.asarray(v, np.float64)).to(dtype) for k, v in inputs.items()}
    total = None
    for l in spec.layers:
        t = l.type
        if t == "Input":
            continue
        x = B[l.bottoms[0]]
        P = params.get(l.name)
        if t == "Convolution":
            k, s, pad = kernel_stride_pad(l.sub("convolution_param"))
            y = F.conv2d(x, P[0], P[1] if len(P) > 1 else None, stride=s, padding=pad)
        elif t == "InnerProduct":
            y = F.linear(x.reshape(x.shape[0], -1), P[0], P[1] if len(P) > 1 else None)
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
                if updates is not None:
                    m, f = x.numel() // x.shape[1], float(l.sub("batch_norm_param").get("moving_average_fraction", 0.999))
                    updates[l.name] = [(P[0] * f + mean).detach().double().numpy(),
                                       (P[1] * f + var * (m / (m - 1.0) if m > 1 else 1.0)).detach().double().numpy(),
                                       (P[2] * f + 1.0).detach().double().numpy()]
            y = (x - _c(mean, x)) / torch.sqrt(_c(var, x) + eps)
        elif t == "Scale" and len(l.bottoms) == 2:
            g = B[l.bottoms[1]]
            y = x * g.reshape(g.shape[0], g.shape[1], *([1] * (x.dim() - 2)))
        elif t == "Scale":
            y = x * _c(P[0], x) + (_c(P[1], x) if len(P) > 1 else 0.0)
        elif t == "ReLU":
            y = torch.relu(x) if relu_masks is None else x * torch.as_tensor(np.asarray(relu_masks[l.name])).to(dtype)
        elif t == "Sigmoid":
            y = torch.sigmoid(x)
        elif t == "Pooling":
            pp = l.sub("pooling_param")
            k, s, pad = (tuple(x.shape[2:]), 1, 0) if bool(pp.get("global_pooling", False)) else kernel_stride_pad(pp)
            y = F.max_pool2d(x, k, s, pad, ceil_mode=True) if str(pp.get("pool", "MAX")) == "MAX" else F.avg_pool2d(x, k, s, pad, ceil_mode=True)
            assert tuple(y.shape) == tuple(spec.blob_shapes[l.tops[0]]), l.name
        elif t == "Eltwise":
            y = x + B[l.bottoms[1]]
        elif t == "Softmax":
            y = torch.softmax(x, dim=1)
        elif t == "SoftmaxWithLoss":
            y = F.cross_entropy(x, B[l.bottoms[1]].reshape(-1).long(), reduction="mean")
            total = y if total is None else total + y
        elif t == "Accuracy":
            lab = B[l.bottoms[1]].reshape(-1).long()
            y = ((x > x.gather(1, lab[:, None])).sum(dim=1) < 1).to(dtype).mean()
        else:
            raise NotImplementedError(t)
        if round_blob is not None:
            y = round_blob(l, l.tops[0], y)
        B[l.tops[0]] = y
    if total is not None:
        B["total_loss"] = total
    return B


def se_params(spec, seed, spread=2.2):
    """tests/torch_resnet_ref.random_params, with the biases of the excite layers (conv*_1x1_up) spread over (-spread, spread): the gates
    then lie all over (0.1, 0.9) - sigmoid(2.2) = 0.9 - instead of around 0.5; what the weights add moves them apart between the images."""
    params = random_params(spec, seed)
    rng = np.random.default_rng(seed + 1)
    for name, blobs in params.items():
        if name.endswith("_1x1_up"):
            blobs[1] = rng.uniform(-spread, spread, blobs[1].shape).astype(np.float32)
    return params


# ---- the net of tests/test_gpu_se_nets.py, shared with its part without a GPU (tests/test_se_nets_ref.py) ------------------------------
KW = dict(depth=50, width_div=8, size=64, batch=2, num_classes=10, reduction=4)      # squeeze widths 8 .. 64: whole groups in both element types
BLOCKS = ["conv%d_%d" % (s, b + 1) for s, n in zip((2, 3, 4, 5), (3, 4, 6, 3)) for b in range(n)]
TOL = 1e-4                                   # the project's rel_err bound for float32 results
MEASURED_F32 = 1.62e-3                       # the float32 run of half_reference against the float64 one (tests/test_gpu_se_nets.py says how)
TOL_F16 = min(4 * MEASURED_F32, 5e-3)        # ... capped by the project's bound for half-float nets


def gates_spread(ref):
    """The gates of every block reach below 0.2 and above 0.8 and differ between the two images."""
    for b in BLOCKS:
        g = ref[b + "_prob"].numpy().reshape(2, -1)
        assert g.min() < 0.2 and g.max() > 0.8, (b, g.min(), g.max())
        assert np.abs(g[0] - g[1]).max() > 0.05, (b, np.abs(g[0] - g[1]).max())


def se_case(phase, form="scale", seed=21, **over):
    """(prototxt text, NetSpec with scale_gate=True after infer(), parameters, inputs) of the small SE-ResNet-50."""
    from fcn_object_detector_amd import models, proto
    from fcn_object_detector_amd.netspec import NetSpec
    txt = models.se_resnet(phase, form=form, **dict(KW, **over))
    spec = NetSpec(proto.parse_text(txt), "TRAIN" if phase == "TRAIN" else "TEST", depthwise=True, ip_gemm=True, scale_gate=True)
    spec.infer()
    params = se_params(spec, seed)
    rng = np.random.default_rng(seed + 7)
    x = {name: (rng.integers(0, KW["num_classes"], shp).astype(np.float32) if name == "label" else rng.standard_normal(shp).astype(np.float32))
         for name, shp in spec.input_shapes.items()}
    x["data"][1] = 3.0 * x["data"][1] + 1.0      # two images of different statistics: their pooled branches, and so their gates, differ
    return txt, spec, params, x


def as_form(params, spec):
    """The same weights in the other form's shapes: (out, in) <-> (out, in, 1, 1) of the squeeze and excite layers."""
    return {k: [np.asarray(a).reshape(shp) for a, shp in zip(v, spec.param_shapes[k])] for k, v in params.items()}


def half_reference(spec, params, x, dtype=torch.float64):
    """The net rounded where the half-float engine rounds (storage.plan_blobs says which blobs are halves): a half blob is rounded when a
    layer writes it - but a BatchNorm is always one launch with the Scale behind it, and the gated Scale one launch with its Eltwise and
    ReLU (its own top is never written), so neither rounds; an in-place ReLU rounds again what is rounded already.  A bank that reads a
    half blob is halves; biases, BatchNorm / Scale blobs and the gates (tops of a Sigmoid) stay float32."""
    from fcn_object_detector_amd import storage as S
    plan = S.plan_blobs(spec, spec.blob_shapes, spec.data_tops(), spec.output_blobs(), True, True, True)
    half = {n for n, e in plan.esize.items() if e == 2}
    r16 = lambda a: np.asarray(a, np.float32).astype(np.float16).astype(np.float32)
    banks = {l.name for l in spec.param_layers() if l.type in ("Convolution", "InnerProduct") and l.bottoms[0] in half}
    p16 = {k: [r16(v[0]) if k in banks else v[0]] + list(v[1:]) for k, v in params.items()}

    def rnd(l, top, y):
        if top not in half or l.type == "BatchNorm" or (l.type == "Scale" and len(l.bottoms) == 2):
            return y
        return y.to(torch.float16).to(dtype)
    with torch.no_grad():
        return torch_se_net(spec, as_torch(p16, dtype=dtype), x, round_blob=rnd, dtype=dtype), half
