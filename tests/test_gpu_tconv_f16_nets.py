"""The group-1 Deconvolution in the half-float engine (NetSpec tconv_f16=True): tiny nets blob by blob against float64 rounded where
the engine rounds, then the published FCN-32s / 16s / 8s nets through caffe.Net in halves against the float32 engine.

The tiny nets are a few layers over `data` (2 x 8 x 11 x 10), run as Engine(NetSpec(msg, "TEST", tconv_f16=True), dtype="f16") with
seeded parameters and inputs, fused and with fuse=False; every blob is read through read_blob and held to
tests/torch_forward_ref.forward_net in float64 under the rounding hooks of tests/test_gpu_forward_plan_paths_f16.py, widened by this
file's rule for the new layer: the bank of a group-1 Deconvolution over halves is halves (storage.param_layout with the keyword), its
bias float32; a blob of halves is rounded each time a layer writes it.  forward() gives the same bits twice and without a graph.

Threshold, measured and not chosen, by the rule of tests/test_gpu_rconv_f16_nets.py: the float32 run of the interpreter with the same
hooks against the float64 one, over the three cases, both plans and three seeds:
    worst rel_err             2.52e-4 (deconvolution_into_the_cropped_float32_output; 2.02e-4 with the skip, 5.2e-5 decoder step): MEASURED_F32
    smallest wrong distance   0.857   (decoder_step_k2s2_with_an_in_place_relu, kh and kw swapped)
TOL = 4 x MEASURED_F32 = 1.01e-3 on rel_err: at most 5e-3, the project's bound for half-float nets.  The part without a GPU measures again, and
shows on the reference alone that each case can fail: two wrong evaluations per case - a wrong phase origin (the two phases of the x
axis trade places) and the taps read with kh and kw swapped - are each at least 10 x TOL away."""
import functools
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec
from test_gpu_forward_plan_paths import FILL, conv, conv1, copies, elt, launch_list, numpy_blobs, pool, relu, same_bits
from test_gpu_forward_plan_paths_f16 import blob_plan, parse, r16, rounding_hooks
from torch_forward_ref import forward_net
from torch_resnet_ref import as_torch, random_params

MEASURED_F32 = 2.52e-4
TOL = 4 * MEASURED_F32
WRONG_AT_LEAST = 10 * TOL
SEEDS = 3
INPUT = 'input: "data" input_shape { dim: 2 dim: 8 dim: 11 dim: 10 }\n'


def deconv(name, bottom, n, k, s):
    return 'layer { name: "%s" type: "Deconvolution" bottom: "%s" top: "%s" convolution_param { num_output: %d kernel_size: %d stride: %d %s } }\n' % (
        name, bottom, name, n, k, s, FILL)


def crop(name, bottom, like, offset):
    return 'layer { name: "%s" type: "Crop" bottom: "%s" bottom: "%s" top: "%s" crop_param { axis: 2 offset: %d } }\n' % (name, bottom, like, name, offset)


def phases_trade_places(y, B, P):
    """A wrong phase origin along x: the outputs of the two phases of a stride-2 layer written to each other's lattice."""
    out = y.clone()
    w = y.shape[3] // 2 * 2
    out[..., 0:w:2], out[..., 1:w:2] = y[..., 1:w:2], y[..., 0:w:2]
    return out


def taps_swapped(layer, bottom, s):
    """The layer with tap (r, q) read where tap (q, r) lies: kh and kw swapped in the bank's index."""
    def patch(y, B, P):
        return F.conv_transpose2d(B[bottom], r16(P[layer][0]).transpose(2, 3), P[layer][1], stride=s)
    return patch


def once(f):
    """A blob that an in-place layer writes again is patched where the Deconvolution wrote it, and then left as it is."""
    calls = []

    def patch(y, B, P):
        calls.append(1)
        return f(y, B, P) if len(calls) == 1 else y
    return patch


# name, body, float32 blobs, the blob the wrong evaluations are judged on, [(what, {blob: patch})]
CASES = [
    ("deconvolution_into_the_cropped_float32_output",
     conv("c0", "data", 5) + deconv("up", "c0", 5, 4, 2) + crop("score", "up", "data", 3), ("data", "score"), "score",
     [("a wrong phase origin", {"up": phases_trade_places}), ("kh and kw swapped", {"up": taps_swapped("up", "c0", 2)})]),
    ("eltwise_skip_as_in_fcn16s",
     conv("c0", "data", 8) + relu("r0", "c0") + pool("p", "c0", 2, 2) + conv1("sfr", "p", 5) + deconv("up2", "sfr", 5, 4, 2) + conv1("sp", "c0", 5)
     + crop("up2c", "up2", "sp", 1) + elt("fuse", ["up2c", "sp"], "operation: SUM") + deconv("up", "fuse", 5, 4, 2) + crop("score", "up", "data", 5),
     ("data", "score"), "score",
     [("a wrong phase origin", {"up2": phases_trade_places}), ("kh and kw swapped", {"up": taps_swapped("up", "fuse", 2)})]),
    ("decoder_step_k2s2_with_an_in_place_relu",
     conv("c0", "data", 16) + relu("r0", "c0") + deconv("d", "c0", 8, 2, 2) + relu("rd", "d") + conv1("u", "d", 8), ("data", "u"), "d",
     [("a wrong phase origin", {"d": phases_trade_places}), ("kh and kw swapped", {"d": taps_swapped("d", "c0", 2)})]),
]
IDS = [c[0] for c in CASES]


def case_inputs(index, spec, seed):
    params = random_params(spec, seed)
    x = np.random.default_rng([seed, 1]).standard_normal(spec.input_shapes["data"]).astype(np.float32)
    return params, {"data": x}


def hooks(spec, plan):
    """The rounding hooks, and: the bank of a group-1 Deconvolution whose bottom holds halves is halves."""
    store, conv_operands = rounding_hooks(spec, plan, {})

    def operands(l, x, P, B):
        if l.type == "Deconvolution" and int(l.sub("convolution_param").get("group", 1)) == 1 and plan.esize[l.bottoms[0]] == 2:
            return x, [r16(P[0])] + list(P[1:])
        return conv_operands(l, x, P, B)
    return store, operands


def evaluate(index, spec, params, x, fused, dtype=torch.float64, wrong=None):
    """Every blob as the half-float engine holds it (numpy float64), by the plan with or without fusion."""
    kw = {}
    P = as_torch(params, dtype=dtype)
    if wrong is not None:
        fresh = {k: once(f) for k, f in CASES[index][4][wrong][1].items()}      # (`d` is written again by its in-place ReLU)
        kw = dict(patch={k: (lambda y, B, f=f: f(y, B, P)) for k, f in fresh.items()})
    plan = blob_plan(spec, fused)
    store, operands = hooks(spec, plan)
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


def wrong_distance(index, which):
    ref = reference(index)
    wrong = evaluate(index, ref["spec"], ref["params"], ref["x"], True, wrong=which)[0]
    blob = CASES[index][3]
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
    wrongs = [wrong_distance(i, j) for i in range(len(CASES)) for j in range(2)]
    print("TCONV16 measured float32 against float64: %s; wrong distances: %s" % (
        " ".join("%s %.3g" % kv for kv in zip(IDS, per_case)), " ".join("%.3g" % w for w in wrongs)))
    assert abs(max(per_case) / MEASURED_F32 - 1) <= 0.1
    assert TOL == 4 * MEASURED_F32 and TOL <= 5e-3


@pytest.mark.parametrize("which", [0, 1], ids=["phase-origin", "kh-kw-swapped"])
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_reference_shows_the_case_can_fail(index, which):
    ref = reference(index)
    assert {n for n, es in ref["plan"].esize.items() if es == 4} == set(CASES[index][2])
    assert set(ref["blobs"]) == set(ref["spec"].blob_shapes) == set(ref["unfused"])
    err = wrong_distance(index, which)
    assert err >= WRONG_AT_LEAST, (CASES[index][4][which][0], err)


def make_engine(ref, **kw):
    from fcn_object_detector_amd.engine import Engine
    eng = Engine(NetSpec(ref["msg"], "TEST", tconv_f16=True), params={k: [a.copy() for a in v] for k, v in ref["params"].items()}, device=0,
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
    name, _body, f32, _blob, _wrong = CASES[index]
    ref = reference(index)
    names = list(ref["spec"].blob_shapes)
    deconvs = [l.name for l in ref["spec"].layers if l.type == "Deconvolution"]
    worst = {}
    eng = make_engine(ref)
    try:
        ll = launch_list(eng)
        for d in deconvs:
            assert ll[ll.index(("tconv_pack", d)) + 1] == ("tconv", d)
            seg = eng.param_segs[(d, 0)]
            assert seg.esize == 2 and seg.shape[-1] % 8 == 0
            assert np.array_equal(eng.read_param(d, 0), ref["params"][d][0].astype(np.float16).astype(np.float32))      # net.params see float32
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
    print("TCONV16 %s %s" % (name, " ".join("%s %.2g" % kv for kv in worst.items())))


@pytest.mark.gpu
def test_a_bare_netspec_still_refuses(gpu):
    from fcn_object_detector_amd.engine import Engine
    ref = reference(0)
    with pytest.raises(NotImplementedError) as ei:
        Engine(NetSpec(ref["msg"], "TEST"), params=ref["params"], device=0, autotune=False, dtype="f16")
    assert str(ei.value) == "f16 engine: layer type Deconvolution with group 1 (up) has no half-float kernel"


# ------------------------------------------------------------------------------------------------------------ through the public door
VALUE_TOL = {"f32": 1e-4, "f16": 5e-3}      # tests/test_gpu_argmax_nets.py
BUILDERS = {32: models.voc_fcn32s, 16: models.voc_fcn16s, 8: models.voc_fcn8s}
SMALL = dict(num_classes=5, shape=(1, 3, 64, 48), width_div=8, fc_div=128, fillers=True)      # VGG widths 8 .. 64, fc6 / fc7 32
# Seeds of the parameters (torch_resnet_ref.random_params) and of the image, chosen so that the float32 margins are clear on at least 95 % of
# the map: the float64 interpreter finds 95.6 % (32s), 95.8 % (16s) and 96.1 % (8s) of the 3072 pixels clear; the float32 engine's own
# share is asserted below.
SEED = {32: 36, 16: 1, 8: 3}
CLEAR_SHARE = 0.95


def published(variant, argmax):
    text = BUILDERS[variant]("TEST", argmax=argmax, **SMALL)
    spec = NetSpec(proto.parse_text(text), "TEST")
    spec.infer()
    params = random_params(spec, SEED[variant])
    x = np.random.default_rng(SEED[variant]).standard_normal(spec.input_shapes["data"]).astype(np.float32)
    return text, spec, params, x


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


def both_engines(tmp_path, monkeypatch, variant, argmax):
    """{dtype: (scores, outputs)} of the net through caffe.Net on the same seeded parameters; the half forward gives the same bits twice."""
    monkeypatch.setenv("FCN_AUTOTUNE", "0")
    text, spec, params, x = published(variant, argmax)
    got = {}
    for dtype in ("f32", "f16"):
        net = caffe_net(tmp_path, text, params, spec, dtype, x)
        try:
            kinds = [op.kind for op in net._engine.ops]
            assert kinds.count("tconv") == {32: 1, 16: 2, 8: 3}[variant] and kinds.count("crop") == {32: 1, 16: 2, 8: 3}[variant]
            if dtype == "f16":
                assert net._engine.f16 and net._engine.blobs["score"].esize == (2 if argmax else 4)
            out = {k: np.array(v) for k, v in net.forward().items()}
            got[dtype] = (np.array(net.blobs["score"].data, np.float64), out)
            if dtype == "f16":
                again = {k: np.array(v) for k, v in net.forward().items()}
                assert all(out[k].tobytes() == again[k].tobytes() for k in out)
        finally:
            net._engine.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [32, 16, 8])
def test_published_fcn_in_halves_through_caffe_net(gpu, tmp_path, monkeypatch, variant):
    got = both_engines(tmp_path, monkeypatch, variant, False)
    (s32, o32), (s16, o16) = got["f32"], got["f16"]
    print("TCONV16 fcn%ds score %.3g" % (variant, rel_err(s16, s32)))
    assert list(o16) == ["score"] and o16["score"].shape == (1, 5, 64, 48) and o16["score"].dtype == np.float32
    assert rel_err(s16, s32) < VALUE_TOL["f16"]


def clear_pixels(s32):
    """Where the float32 margin between the best two classes exceeds twice the allowance of a score."""
    top = np.sort(s32, axis=1)
    return (top[:, -1] - top[:, -2]) > 2 * VALUE_TOL["f16"] * np.abs(s32).max()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [32, 16, 8])
def test_published_fcn_label_maps_in_halves(gpu, tmp_path, monkeypatch, variant):
    got = both_engines(tmp_path, monkeypatch, variant, True)
    (s32, o32), (s16, o16) = got["f32"], got["f16"]
    assert list(o16) == ["argmax"] and o16["argmax"].shape == (1, 1, 64, 48)
    assert rel_err(s16, s32) < VALUE_TOL["f16"]
    clear = clear_pixels(s32)
    print("TCONV16 fcn%ds clear margins: %d of %d" % (variant, clear.sum(), clear.size))
    assert clear.mean() >= CLEAR_SHARE
    assert np.array_equal(o32["argmax"][:, 0], s32.argmax(axis=1))
    assert np.array_equal(o32["argmax"][:, 0][clear], o16["argmax"][:, 0][clear])
