"""Forward values on the CPU for the plan matrix of tests/test_gpu_forward_plan_paths.py: one torch interpreter of a NetSpec, float64 unless
told otherwise, independent of the engine.  It runs the layers in the order of the prototxt, which is what Caffe does.

The layer types of tests/torch_fanout_ref.torch_net that the matrix uses (Convolution with groups, InnerProduct, ReLU with a slope, Sigmoid,
LRN, BatchNorm with batch or global statistics, Scale, Concat, and the two poolings by Caffe's own rules: that file's max_pool_caffe), plus

    Power      (shift + scale * x) ** power
    Slice      along axis 1 at slice_point (equal parts without one)
    Dropout    the identity in TEST; refused in TRAIN (the matrix has no such layer)
    Softmax    along axis 1
    Eltwise    PROD, MAX, and SUM with coeff
and, for the half-float matrix of tests/test_gpu_forward_plan_paths_f16.py,
    DepthwiseConvolution          one filter per channel
    Deconvolution                 conv_transpose2d with convolution_param's group
    Crop, Interp                  as tests/torch_fanout_ref.py has them
    Upsample                      the scatter by the pooling's argmax (windows that share no pixel)
    Pooling with global_pooling   the mean or the maximum of the plane

forward_net returns (B, first, seen, top2): B every blob at its FINAL value, a pooling mask as the int64 index max_pool_caffe computes;
first[blob] the value a blob held before the first in-place layer overwrote it; seen[layer] what a layer read as its first bottom;
top2[MAX pooling layer] the two largest values of every window.

Three hooks state a WRONG evaluation, for the tests that show a case can fail:
    patch      {blob: f}: the blob is replaced by f(value, B) each time a layer has written it - everything downstream reads the patched value
    pad_value  {Convolution layer: v}: its padding holds v, not 0
    bn_global  {BatchNorm layer: bool}: global statistics (True) or batch statistics (False), whatever the phase says
A mutated layer list is a mutated prototxt: the caller parses another text and passes the same parameters.

Two more hooks state where an engine ROUNDS (the half-float engine); without them nothing changes, bit for bit:
    store      f(name, y) -> y, applied to every blob each time a layer (or the caller, for an input) writes it, ahead of `patch`; an
               Eltwise over more than two bottoms passes its partial results through it as well - the engine's launches are pairwise and
               keep the partial result in the top
    operands   f(layer, x, P, B) -> (x, P), applied to the first bottom and the parameter blobs of a Convolution, DepthwiseConvolution,
               InnerProduct or Deconvolution ahead of the arithmetic: the banks the device keeps in another number format, or an input
               it keeps in another form (the half image with its two constant channels)"""
import numpy as np
import torch
import torch.nn.functional as F

from fcn_object_detector_amd.netspec import bn_global_stats, crop_window, layer_dilation, layer_geometry
from torch_fanout_ref import _c, max_pool_caffe
from torch_interp_ref import interp

INPUT_TYPES = ("Input", "Python", "Data")


def slice_edges(l, channels):
    sp = l.sub("slice_param")
    pts = [int(p) for p in sp.getall("slice_point")] or [channels // len(l.tops) * i for i in range(1, len(l.tops))]
    return [0] + pts + [channels]


def eltwise(l, xs, partial=None):
    p = l.sub("eltwise_param")
    op = str(p.get("operation", "SUM"))
    if partial is not None:      # pairwise, as the engine launches it: (ca a + cb b), then (1 y + cc c), ... - each partial result stored
        coeff = [float(c) for c in p.getall("coeff")] or [1.0] * len(xs)
        assert op in ("PROD", "MAX", "SUM") and len(coeff) == len(xs)
        y = xs[0]
        for i, x in enumerate(xs[1:], start=1):
            if op == "SUM":
                y = (coeff[0] if i == 1 else 1.0) * y + coeff[i] * x
            else:
                y = y * x if op == "PROD" else torch.maximum(y, x)
            if i < len(xs) - 1:
                y = partial(y)
        return y
    if op == "PROD":
        y = xs[0]
        for x in xs[1:]:
            y = y * x
        return y
    if op == "MAX":
        y = xs[0]
        for x in xs[1:]:
            y = torch.maximum(y, x)
        return y
    assert op == "SUM", op
    coeff = [float(c) for c in p.getall("coeff")] or [1.0] * len(xs)
    assert len(coeff) == len(xs)
    return sum(c * x for c, x in zip(coeff, xs))


def forward_net(spec, params, inputs, dtype=torch.float64, patch=None, pad_value=None, bn_global=None, store=None, operands=None):
    patch, pad_value, bn_global = patch or {}, pad_value or {}, bn_global or {}
    B, first, seen, top2 = {}, {}, {}, {}

    def write(name, y):
        if name in B and name not in first:
            first[name] = B[name]
        if store is not None and y.dtype == dtype:      # (a pooling mask is an index, not a value)
            y = store(name, y)
        B[name] = patch[name](y, B) if name in patch else y

    for k, v in inputs.items():
        write(k, torch.as_tensor(np.asarray(v, np.float64)).to(dtype))
    for l in spec.layers:
        t = l.type
        if t in INPUT_TYPES:
            continue
        x = seen[l.name] = B[l.bottoms[0]]
        P = params.get(l.name)
        if operands is not None and t in ("Convolution", "DepthwiseConvolution", "InnerProduct", "Deconvolution"):
            x, P = operands(l, x, P, B)
        if t == "Convolution" or t == "DepthwiseConvolution":
            kh, kw, sh, sw, ph, pw = layer_geometry(l)
            if l.name in pad_value:
                x, ph, pw = F.pad(x, (pw, pw, ph, ph), value=float(pad_value[l.name])), 0, 0
            y = F.conv2d(x, P[0], P[1] if len(P) > 1 else None, stride=(sh, sw), padding=(ph, pw), dilation=layer_dilation(l),
                         groups=x.shape[1] if t == "DepthwiseConvolution" else int(l.sub("convolution_param").get("group", 1)))
        elif t == "Deconvolution":
            kh, kw, sh, sw, ph, pw = layer_geometry(l)
            y = F.conv_transpose2d(x, P[0], P[1] if len(P) > 1 else None, stride=(sh, sw), padding=(ph, pw),
                                   groups=int(l.sub("convolution_param").get("group", 1)))
        elif t == "InnerProduct":
            y = F.linear(x.reshape(x.shape[0], -1), P[0], P[1] if len(P) > 1 else None)
        elif t == "ReLU":
            y = torch.where(x > 0, x, float(l.sub("relu_param").get("negative_slope", 0.0)) * x)
        elif t == "Sigmoid":
            y = torch.sigmoid(x)
        elif t == "Power":
            p = l.sub("power_param")
            y = (float(p.get("shift", 0.0)) + float(p.get("scale", 1.0)) * x) ** float(p.get("power", 1.0))
        elif t == "Dropout":
            assert spec.phase == "TEST", "Dropout in TRAIN draws a mask: not a layer of this matrix"
            y = x
        elif t == "Softmax":
            assert int(l.sub("softmax_param").get("axis", 1)) == 1
            y = torch.softmax(x, dim=1)
        elif t == "Pooling":
            pp = l.sub("pooling_param")
            if bool(pp.get("global_pooling", False)):
                y = x.amax(dim=(2, 3), keepdim=True) if str(pp.get("pool", "MAX")) == "MAX" else x.mean(dim=(2, 3), keepdim=True)
                assert tuple(y.shape) == tuple(spec.blob_shapes[l.tops[0]]), l.name
                write(l.tops[0], y)
                continue
            kh, kw, sh, sw, ph, pw = layer_geometry(l)
            assert (kh, sh, ph) == (kw, sw, pw)
            if str(pp.get("pool", "MAX")) == "MAX":
                y, idx, top2[l.name] = max_pool_caffe(x, kh, sh, ph)
                if len(l.tops) > 1:
                    write(l.tops[1], idx)
            else:
                y = F.avg_pool2d(x, kh, sh, ph, ceil_mode=True, count_include_pad=True)
        elif t == "LRN":
            p = l.sub("lrn_param")
            y = F.local_response_norm(x, int(p.get("local_size", 5)), float(p.get("alpha", 1.0)), float(p.get("beta", 0.75)), float(p.get("k", 1.0)))
        elif t == "BatchNorm":
            eps = float(l.sub("batch_norm_param").get("eps", 1e-5))
            if bn_global.get(l.name, bn_global_stats(l, spec.phase)):
                fac = float(P[2].reshape(-1)[0])
                sc = 0.0 if fac == 0.0 else 1.0 / fac
                mean, var = sc * P[0], sc * P[1]
            else:
                dims = [d for d in range(x.dim()) if d != 1]
                mean = x.mean(dim=dims)
                var = ((x - _c(mean, x)) ** 2).mean(dim=dims)
            y = (x - _c(mean, x)) / torch.sqrt(_c(var, x) + eps)
        elif t == "Scale":
            y = x * _c(P[0], x)
            if len(P) > 1:
                y = y + _c(P[1], x)
        elif t == "Eltwise":
            y = eltwise(l, [B[b] for b in l.bottoms], None if store is None else lambda v: store(l.tops[0], v))
        elif t == "Crop":
            shape, (_, oc, oy, ox) = crop_window(l, tuple(x.shape), tuple(B[l.bottoms[1]].shape))
            y = x[:, oc:oc + shape[1], oy:oy + shape[2], ox:ox + shape[3]]
        elif t == "Interp":
            y = interp(x, l)
        elif t == "Upsample":
            n, c, h, w = spec.blob_shapes[l.tops[0]]
            idx = B[l.bottoms[1]]
            assert idx.dtype == torch.int64 and tuple(idx.shape) == tuple(x.shape)
            assert all(len(set(v.tolist())) == v.numel() for v in idx.flatten(2).flatten(0, 1)), "two windows share a pixel"
            y = torch.zeros((n, c, h * w), dtype=dtype).scatter(2, idx.flatten(2), x.flatten(2)).reshape(n, c, h, w)
        elif t == "Concat":
            y = torch.cat([B[b] for b in l.bottoms], dim=1)
        elif t == "Slice":
            edges = slice_edges(l, x.shape[1])
            assert len(edges) == len(l.tops) + 1
            for tp, a, b in zip(l.tops, edges[:-1], edges[1:]):
                assert tuple(x[:, a:b].shape) == tuple(spec.blob_shapes[tp]), l.name
                write(tp, x[:, a:b])
            continue
        else:
            raise NotImplementedError(t)
        assert tuple(y.shape) == tuple(spec.blob_shapes[l.tops[0]]), l.name
        write(l.tops[0], y)
    return B, first, seen, top2
