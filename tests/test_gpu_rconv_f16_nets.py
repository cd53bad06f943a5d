"""Dilated and rectangular Convolution in the half-float engine (NetSpec rconv_f16=True): tiny nets blob by blob against float64
rounded where the engine rounds, then DeepLab-LargeFOV and Inception-v3 through caffe.Net against the float32 engine.

The tiny nets are a few layers over `data` (2 x 8 x 11 x 10), run as Engine(NetSpec(msg, "TEST", rconv_f16=True), dtype="f16") with
seeded parameters and inputs, fused and with fuse=False; every blob is read through read_blob and held to
tests/torch_forward_ref.forward_net in float64 under the rounding hooks of tests/test_gpu_forward_plan_paths_f16.py (a blob of halves
is rounded each time a layer writes it, the filters of a Convolution over halves are halves, biases stay float32).  forward() gives
the same bits twice and without a graph.

Threshold, measured and not chosen, by that module's rule: the float32 run of the interpreter with the same hooks against the float64
one, over the four cases, both plans and three seeds:
    worst rel_err             1.41e-4 (a_dilated_layer_between_dense_ones, two_dilations_into_a_concat): MEASURED_F32
    smallest wrong distance   1.25    (two_dilations_into_a_concat)
TOL = 4 x MEASURED_F32 = 5.64e-4 on rel_err: at most 5e-3, the project's bound for half-float nets.  The part without a GPU measures
again, and shows on the reference alone that each case can fail: one wrong evaluation per case (the dilation dropped, the pads of the
two axes swapped, the float32 output rounded to halves - with filters scaled so that it leaves the half range) is at least 10 x TOL
away."""
import functools
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec
from test_gpu_forward_plan_paths import concat, conv, conv1, copies, launch_list, numpy_blobs, relu, same_bits
from test_gpu_forward_plan_paths_f16 import blob_plan, parse, r16, rounding_hooks
from torch_forward_ref import forward_net
from torch_resnet_ref import as_torch, random_params

MEASURED_F32 = 1.41e-4
TOL = 4 * MEASURED_F32
WRONG_AT_LEAST = 10 * TOL
SEEDS = 3
INPUT = 'input: "data" input_shape { dim: 2 dim: 8 dim: 11 dim: 10 }\n'
C0 = conv("c0", "data", 8)
D2, D3 = "kernel_size: 3 pad: 2 dilation: 2", "kernel_size: 3 pad: 3 dilation: 3"
K17, K71 = "kernel_h: 1 kernel_w: 7 pad_h: 0 pad_w: 3", "kernel_h: 7 kernel_w: 1 pad_h: 3 pad_w: 0"


def shifted_by_swapped_pads(layer, bottom, kh, kw, ph, pw):
    """The layer evaluated with the pads of its two axes swapped - tap (r, q) of pixel (i, j) reads x[i - pw + r, j - ph + q] - on the
    layer's own output grid."""
    def patch(y, B, P):
        big = 2 * max(ph, pw)
        full = F.conv2d(F.pad(B[bottom], (big, big, big, big)), r16(P[layer][0]), P[layer][1])
        return full[:, :, big - pw:big - pw + y.shape[2], big - ph:big - ph + y.shape[3]]
    return patch


# name, body, launches (fused), float32 blobs, tweak, wrong: (what, blob, replace or None, patch or None)
CASES = [
    ("a_dilated_layer_between_dense_ones", C0 + conv("k", "c0", 8, D2) + conv("u", "k", 8), "conv:c0 | dconv:k | conv:u", ("data", "u"), None,
     ("the dilation dropped", "k", ("pad: 2 dilation: 2", "pad: 1"), None)),
    ("the_pair_1x7_7x1", C0 + conv("a", "c0", 8, K17) + relu("ar", "a") + conv("b", "a", 8, K71) + relu("br", "b") + conv1("u", "b", 8),
     "conv:c0 | rconv:a | rconv:b | conv:u", ("data", "u"), None,
     ("the pads of the two axes swapped", "a", None, {"a": shifted_by_swapped_pads("a", "c0", 1, 7, 0, 3)})),
    ("two_dilations_into_a_concat", C0 + conv("a", "c0", 8, D2) + conv("b", "c0", 8, D3) + concat("cat", ["a", "b"]) + conv1("u", "cat", 8),
     "conv:c0 | dconv:a+b | conv:u", ("data", "u"), None,
     ("the dilation of the second member dropped", "cat", ("pad: 3 dilation: 3", "pad: 1"), None)),
    ("a_dilated_layer_as_the_float32_output", C0 + conv("u", "c0", 8, D2), "conv:c0 | dconv:u", ("data", "u"), ("u", 3e4),
     ("the float32 output rounded to halves", "u", None, {"u": lambda y, B, P: r16(y)})),
]
IDS = [c[0] for c in CASES]


def case_inputs(index, spec, seed):
    params = random_params(spec, seed)
    tweak = CASES[index][4]
    if tweak is not None:
        for a in params[tweak[0]]:
            a *= np.float32(tweak[1])
    x = np.random.default_rng([seed, 1]).standard_normal(spec.input_shapes["data"]).astype(np.float32)
    return params, {"data": x}


def evaluate(index, spec, params, x, fused, dtype=torch.float64, wrong=False):
    """Every blob as the half-float engine holds it (numpy float64), by the plan with or without fusion."""
    text = INPUT + CASES[index][1]
    kw = {}
    P = as_torch(params, dtype=dtype)
    if wrong:
        _what, _blob, replace, patch = CASES[index][5]
        if replace is not None:
            assert text.count(replace[0]) == 1
            spec = parse(text.replace(*replace))[1]
        if patch is not None:
            kw = dict(patch={k: (lambda y, B, f=f: f(y, B, P)) for k, f in patch.items()})
    plan = blob_plan(spec, fused)
    store, operands = rounding_hooks(spec, plan, {})
    blobs = numpy_blobs(forward_net(spec, P, x, dtype=dtype, store=store, operands=operands, **kw)[0])
    for name in blobs:
        if plan.esize.get(name, 4) == 2:
            blobs[name] = blobs[name].astype(np.float16).astype(np.float64)
    blobs["data"] = np.asarray(x["data"], np.float64)
    return blobs, plan


@functools.lru_cache(maxsize=None)
def reference(index):
    """Case `index`, computed once and shared by the tests."""
    msg, spec = parse(INPUT + CASES[index][1])
    params, x = case_inputs(index, spec, 1)
    fused, plan = evaluate(index, spec, params, x, True)
    unfused, _ = evaluate(index, spec, params, x, False)
    return dict(msg=msg, spec=spec, params=params, x=x, blobs=fused, unfused=unfused, plan=plan)


def worst_wrong(index):
    ref = reference(index)
    wrong = evaluate(index, ref["spec"], ref["params"], ref["x"], True, wrong=True)[0]
    blob = CASES[index][5][1]
    return rel_err(wrong[blob], ref["blobs"][blob])


@functools.lru_cache(maxsize=None)
def measurement():
    """Worst rel_err of the float32 interpreter against the float64 one, both under the hooks, per case over both plans and three seeds."""
    out = []
    for index in range(len(CASES)):
        spec = reference(index)["spec"]
        worst = 0.0
        for k in range(SEEDS):
            params, x = case_inputs(index, spec, 1 + 100 * k)
            for fused in (True, False):
                want = evaluate(index, spec, params, x, fused)[0]
                got = evaluate(index, spec, params, x, fused, dtype=torch.float32)[0]
                worst = max(worst, max(rel_err(got[n], want[n]) for n in want))
        out.append(worst)
    return out


def test_threshold_is_the_measured_one():
    per_case = measurement()
    wrongs = [worst_wrong(i) for i in range(len(CASES))]
    print("RCONV16 measured float32 against float64: %s; wrong distances: %s" % (
        " ".join("%s %.3g" % kv for kv in zip(IDS, per_case)), " ".join("%.3g" % w for w in wrongs)))
    assert abs(max(per_case) / MEASURED_F32 - 1) <= 0.1
    assert TOL == 4 * MEASURED_F32 and TOL <= 5e-3


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_reference_shows_the_case_can_fail(index):
    ref = reference(index)
    assert {n for n, es in ref["plan"].esize.items() if es == 4} == set(CASES[index][3])
    assert set(ref["blobs"]) == set(ref["spec"].blob_shapes) == set(ref["unfused"])
    err = worst_wrong(index)
    assert err >= WRONG_AT_LEAST, (CASES[index][5][0], err)


def make_engine(ref, **kw):
    from fcn_object_detector_amd.engine import Engine
    eng = Engine(NetSpec(ref["msg"], "TEST", rconv_f16=True), params={k: [a.copy() for a in v] for k, v in ref["params"].items()}, device=0,
                 autotune=False, dtype="f16", **kw)
    eng.host_array("data")[...] = ref["x"]["data"]
    return eng


def compare(eng, want, names, worst):
    for name in names:
        got = eng.read_blob(name)
        assert got.shape == want[name].shape, name
        worst[name] = max(worst.get(name, 0.0), rel_err(got, want[name]))
        assert worst[name] < TOL, (name, worst[name])


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_tiny_net_in_halves(gpu, index):
    name, _body, launches, f32, _tweak, _wrong = CASES[index]
    ref = reference(index)
    names = list(ref["spec"].blob_shapes)
    worst = {}
    eng = make_engine(ref)
    try:
        assert launch_list(eng) == [tuple(s.split(":", 1)) for s in launches.split(" | ")]
        assert {n: b.esize for n, b in eng.blobs.items()} == {n: 4 if n in f32 else 2 for n in names}
        first = copies(eng.forward())
        compare(eng, ref["blobs"], names, worst)
        assert same_bits(first, copies(eng.forward()))
        assert same_bits(first, copies(eng.forward(use_graph=False)))
    finally:
        eng.close()
    eng = make_engine(ref, fuse=False)
    try:
        eng.forward()
        compare(eng, ref["unfused"], names, worst)
    finally:
        eng.close()
    print("RCONV16 %s %s" % (name, " ".join("%s %.2g" % kv for kv in worst.items())))


# ------------------------------------------------------------------------------------------------------------ through the public door
VALUE_TOL = {"f32": 1e-4, "f16": 5e-3}      # tests/test_gpu_argmax_nets.py


def caffe_net(tmp_path, text, params, spec, dtype, x):
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    path, weights = str(tmp_path / "deploy.prototxt"), str(tmp_path / "w.caffemodel")
    open(path, "w").write(text)
    proto.write_caffemodel(weights, [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    caffe.set_device(0)
    caffe.set_mode_gpu()
    net = caffe.Net(path, weights, caffe.TEST, dtype=dtype)
    net.blobs["data"].data[...] = x
    return net


def both_engines(tmp_path, monkeypatch, text, random_params_, seed, scores):
    """(float32 scores, half scores, float32 outputs, half outputs) of the net through caffe.Net on the same seeded parameters; the half
    forward gives the same bits twice and without a graph."""
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    spec = NetSpec(proto.parse_text(text), "TEST")
    spec.infer()
    params = random_params_(spec, seed)
    x = np.random.default_rng(seed).standard_normal(spec.input_shapes["data"]).astype(np.float32)
    got = {}
    for dtype in ("f32", "f16"):
        net = caffe_net(tmp_path, text, params, spec, dtype, x)
        try:
            if dtype == "f16":
                assert net._engine.f16 and {"dconv", "rconv"} & {op.kind for op in net._engine.ops}
            out = {k: np.array(v) for k, v in net.forward().items()}
            got[dtype] = (np.array(net.blobs[scores].data, np.float64), out)
            if dtype == "f16":
                again = {k: np.array(v) for k, v in net.forward().items()}
                plain = {k: np.array(v) for k, v in net._engine.forward(use_graph=False).items()}
                assert all(out[k].tobytes() == again[k].tobytes() == plain[k].tobytes() for k in out)
        finally:
            net._engine.close()
    return got["f32"][0], got["f16"][0], got["f32"][1], got["f16"][1]


def labels_agree(s32, lab32, lab16, axis=1):
    """Equal labels wherever the float32 margin between the best two classes exceeds twice the allowance of a score."""
    top = np.sort(s32, axis=axis)
    margin = np.take(top, -1, axis=axis) - np.take(top, -2, axis=axis)
    clear = margin > 2 * VALUE_TOL["f16"] * np.abs(s32).max()
    print("RCONV16 clear margins: %d of %d" % (clear.sum(), clear.size))
    return np.array_equal(np.asarray(lab32).reshape(clear.shape)[clear], np.asarray(lab16).reshape(clear.shape)[clear])


@pytest.mark.gpu
def test_deeplab_largefov_in_halves_through_caffe_net(gpu, tmp_path, monkeypatch):
    from torch_interp_ref import random_params as rp
    text = models.deeplab_largefov("DEPLOY", num_classes=5, width_div=8, fc_div=8, size=65, interp=True, argmax=True)
    s32, s16, o32, o16 = both_engines(tmp_path, monkeypatch, text, rp, 5, "fc8_interp")
    print("RCONV16 largefov fc8_interp %.3g" % rel_err(s16, s32))
    assert rel_err(s16, s32) < VALUE_TOL["f16"]
    assert list(o16) == ["argmax"] and o16["argmax"].shape == (1, 1, 65, 65)
    assert labels_agree(s32, o32["argmax"][:, 0], o16["argmax"][:, 0])


@pytest.mark.gpu
def test_inception_v3_in_halves_through_caffe_net(gpu, tmp_path, monkeypatch):
    from torch_rect_ref import random_params as rp
    text = models.inception_v3("DEPLOY", batch=2, classes=6, width_div=4, size=75)
    s32, s16, o32, o16 = both_engines(tmp_path, monkeypatch, text, rp, 3, "classifier")
    print("RCONV16 inception_v3 classifier %.3g prob %.3g" % (rel_err(s16, s32), rel_err(o16["prob"], o32["prob"])))
    assert rel_err(s16, s32) < VALUE_TOL["f16"] and rel_err(o16["prob"], o32["prob"]) < VALUE_TOL["f16"]
    assert labels_agree(s32, s32.argmax(axis=1), s16.argmax(axis=1))
