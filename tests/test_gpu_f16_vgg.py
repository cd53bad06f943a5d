"""Half-float inference of the VGG16 nets (`Engine(dtype="f16")` on train/fcn_bbox's deploy form and train/bounding_box/deploy.prototxt),
-m gpu: net level against the oracle rounded at the same points, the detector on the float32 head blobs, the pycaffe front end, graph
replay, and the float32-in / halves-out convolution (FCN_CONV_OUT_F16) that conv1_1 takes because VGG has no Power layer in front."""
import ctypes as C
import sys

import numpy as np
import pytest

from conftest import PYCAFFE, elem_err, rel_err
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.detector import DetectorPipeline, FCNObjectDetector, HeadMapping
from fcn_object_detector_amd.engine import Engine
from fcn_object_detector_amd.netspec import NetSpec, fill_params
from gpu_util import Guards, conv_desc, pack_ohwi, poisoned, poisoned_nhwc, slice_untouched
from oracle import caffe_ref as R
from oracle import detect_ref as D
from oracle.net_ref import RefNet

pytestmark = pytest.mark.gpu


def r16(a):
    return a.astype(np.float16).astype(np.float32)


def build(txt, seed, dtype="f16", **kw):
    msg = proto.parse_text(txt)
    spec = NetSpec(msg, "TEST")
    spec.infer()
    params = fill_params(spec, seed=seed)
    eng = Engine(NetSpec(msg, "TEST"), params={k: [a.copy() for a in v] for k, v in params.items()}, device=0, autotune=False, dtype=dtype, **kw)
    return msg, spec, params, eng


def rounded_oracle(msg, spec, params, eng, x):
    """The oracle with the engine's rounding points: filters of every convolution that reads a half blob are halves (conv1_1 reads the
    float32 image and keeps float32 filters, the bilinear taps of the deconvolutions stay float32), every half blob is rounded when
    it is stored, float32 blobs are not."""
    conv_half = {l.name for l in spec.layers if l.type == "Convolution" and eng.blobs[l.bottoms[0]].esize == 2}
    p16 = {k: [r16(v[0]) if k in conv_half else v[0].copy()] + [a.copy() for a in v[1:]] for k, v in params.items()}
    ref = RefNet(msg, "TEST", p16)
    ref.blobs["data"] = x
    ref.round_activations = lambda name, a: r16(a) if eng.blobs[name].esize == 2 else a
    return ref.forward()


@pytest.mark.parametrize("batch,classes", [(1, 4), (2, 11)])
def test_fcn_bbox_deploy_f16_matches_the_rounded_oracle(gpu, batch, classes):
    msg, spec, params, eng = build(models.vgg16_fcn_bbox_deploy(batch, 96, 64, classes), seed=7)
    wide = sorted(n for n, b in eng.blobs.items() if b.esize == 4)
    assert wide == ["data", "pool_score", "upscore_pool3", "upscore_pool5_bbox"]      # what enters and what the decode kernels read
    kinds = [op.kind for op in eng.ops]
    assert kinds.count("deconv") == 4 and kinds.count("eltwise") == 2 and kinds.count("softmax") == 1
    x = np.random.default_rng(0).random((batch, 3, 96, 64), dtype=np.float32)
    eng.host_array("data")[...] = x
    out = eng.forward()
    rb = rounded_oracle(msg, spec, params, eng, x)
    for name in ("pool_score", "upscore_pool5_bbox", "upscore_pool3"):
        got = eng.read_blob(name)
        worst, at = elem_err(got, rb[name], 5e-3)
        print("F16NET %s rel %.3g elem %.3g" % (name, rel_err(got, rb[name]), worst))
        assert got.dtype == np.float32 and rel_err(got, rb[name]) < 5e-3, name
        assert worst <= 1.0, (name, worst, at)
        assert np.array_equal(out[name], got)
    for name in ("pool3", "score_conv5", "fuse_pool4", "fuse_pool3"):      # half blobs read back as float32 NCHW
        assert rel_err(eng.read_blob(name), rb[name]) < 5e-3, name
    assert np.abs(out["pool_score"].sum(axis=1) - 1.0).max() < 1e-5
    eng.close()


def test_bounding_box_deploy_f16_pyramid_pooling(gpu):
    msg, spec, params, eng = build(models.vgg16_bounding_box_deploy(1, 448, 448, 3), seed=3)
    kinds = [op.kind for op in eng.ops]
    assert kinds.count("avepool") == 4 and kinds.count("deconv") == 4 and kinds.count("copy") == 6
    assert eng.blobs["conv4_3/conv5_3/concat"].esize == 2 and eng.blobs["bboxes"].esize == 4 and eng.blobs["coverage"].esize == 4
    x = np.random.default_rng(2).random((1, 3, 448, 448), dtype=np.float32)
    eng.host_array("data")[...] = x
    out = eng.forward()
    rb = rounded_oracle(msg, spec, params, eng, x)
    assert eng.shapes["conv4_3/conv5_3/concat"] == (1, 1536, 28, 28)
    for name in ("pool4/1x1", "conv4_3/2x2", "conv4_3/4x4/upsample", "conv4_3/1x1/upsample", "conv5_3", "conv4_3/conv5_3/concat", "coverage", "bboxes"):
        got = eng.read_blob(name)
        print("F16NET %s rel %.3g" % (name, rel_err(got, rb[name])))
        assert rel_err(got, rb[name]) < 5e-3, name
    for name in ("coverage", "bboxes"):
        assert np.array_equal(out[name], eng.read_blob(name))
    eng.close()


def _detecting_params(params, classes, rng):
    """Random weights emit no detections: class 1 wins the softmax on most cells and every cell votes for a similar rect."""
    params["score_pool3"][1][1] = 6.0
    params["score_conv5_bbox"][0][...] = 0
    params["score_conv5_bbox"][1][...] = np.tile(np.array([-30, -25, 35, 40], np.float32), classes) + rng.normal(0, 0.5, 4 * classes).astype(np.float32)


@pytest.mark.parametrize("batch", [1, 4])
def test_detector_on_the_f16_fcn_bbox_engine(gpu, batch):
    classes, h, w = 4, 128, 160
    msg = proto.parse_text(models.vgg16_fcn_bbox_deploy(batch, h, w, classes))
    spec = NetSpec(msg, "TEST")
    spec.infer()
    params = fill_params(spec, seed=11)
    rng = np.random.default_rng(3)
    _detecting_params(params, classes, rng)
    eng = Engine(NetSpec(msg, "TEST"), params=params, device=0, autotune=False, dtype="f16")
    det = FCNObjectDetector(eng, 0.5, 3, 0.2)
    assert (det.mapping.cvg_blob, det.mapping.bbox_blob, det.mapping.stride, det.mapping.skip_background) == ("pool_score", "upscore_pool5_bbox", 8, True)
    assert eng.blobs["pool_score"].esize == 4 and eng.blobs["upscore_pool5_bbox"].esize == 4
    frames = [rng.integers(0, 256, fs, dtype=np.uint8) for fs in ((h, w, 3), (240, 352, 3), (100, 217, 3), (300, 200, 3))][:batch]
    res = det.run_detector_batch(frames) if batch > 1 else [det.run_detector(frames[0])]
    score, bb = eng.read_blob("pool_score").copy(), eng.read_blob("upscore_pool5_bbox").copy()
    total = 0
    for i, (frame, (boxes, labels)) in enumerate(zip(frames, res)):
        rdet, rlab = D.detect(score[i, 1:], bb[i], w, h, 8, 0.5, 3, 0.2, fast=True)
        rbox = np.asarray(rdet, dtype=np.int64).reshape(-1, 5)
        if len(rbox):
            rbox = D.resize_detection(frame.shape, rbox, w, h)
        assert np.array_equal(boxes, rbox) and np.array_equal(labels, rlab), i      # integer work on the engine's own maps: bit-exact
        total += len(boxes)
    assert total > 0
    eng.close()


def test_detector_pipeline_on_f16_engines_equals_frame_by_frame(gpu):
    classes, h, w = 4, 128, 160
    msg = proto.parse_text(models.vgg16_fcn_bbox_deploy(1, h, w, classes))
    spec = NetSpec(msg, "TEST")
    spec.infer()
    params = fill_params(spec, seed=11)
    rng = np.random.default_rng(4)
    _detecting_params(params, classes, rng)
    make = lambda first: Engine(NetSpec(msg, "TEST"), params=params, device=0, autotune=False, dtype="f16", tune_from=first)
    lone = FCNObjectDetector(make(None), 0.5, 3, 0.2)
    pipe = DetectorPipeline(make, depth=2, detection_threshold=0.5, min_boxes=3, nms_eps=0.2)
    frames = [rng.integers(0, 256, fs, dtype=np.uint8) for fs in ((h, w, 3), (240, 352, 3), (100, 217, 3), (h, w, 3))]
    want = [lone.run_detector(f) for f in frames]
    got = []
    pipe.submit(frames[0])
    for f in frames[1:]:
        pipe.submit(f)              # two frames in flight
        got.append(pipe.collect())
    got.append(pipe.collect())
    assert sum(len(b) for b, _l in want) > 0
    for (gb, gl), (wb, wl) in zip(got, want):
        assert np.array_equal(gb, wb) and np.array_equal(gl, wl)
    for d in pipe.detectors:
        d.engine.close()
    lone.engine.close()


def test_pycaffe_front_end_builds_the_f16_vgg_net(gpu, tmp_path, monkeypatch):
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    path = str(tmp_path / "deploy.prototxt")
    with open(path, "w") as f:
        f.write(models.vgg16_fcn_bbox_deploy(1, 64, 96, 4))
    caffe.set_device(0)
    caffe.set_mode_gpu()
    x = np.random.default_rng(2).random((1, 3, 64, 96)).astype(np.float32)
    outs = []
    for how in ("keyword", "environment"):
        if how == "keyword":
            net = caffe.Net(path, caffe.TEST, dtype="f16")
        else:
            monkeypatch.setenv("FCN_DTYPE", "f16")
            net = caffe.Net(path, caffe.TEST)
        assert net._engine.f16 and net._engine.blobs["conv3_3"].esize == 2
        net.blobs["data"].data[...] = x
        out = net.forward()
        score = net.blobs["pool_score"].data
        assert score.dtype == np.float32 and score.shape == (1, 4, 8, 12) and np.abs(score.sum(axis=1) - 1).max() < 1e-5
        assert net.blobs["fuse_pool3"].data.dtype == np.float32 and np.array_equal(out["pool_score"], score)
        outs.append((score.copy(), net.blobs["upscore_pool5_bbox"].data.copy()))
        net._engine.close()
    # both ways build the same engine (each tunes its own tile plan: the float32 sums may be ordered differently)
    for a, b in zip(*outs):
        assert rel_err(a, b) < 5e-3
    net32 = caffe.Net(path, caffe.TEST, dtype="f32")
    net32.blobs["data"].data[...] = x
    net32.forward()
    assert rel_err(outs[0][0], net32.blobs["pool_score"].data) < 2e-2      # half storage of 16 layers against pure float32
    net32._engine.close()


def test_graph_replay_equals_plain_launches_bit_for_bit(gpu, monkeypatch):
    txt = models.vgg16_bounding_box_deploy(1, 448, 448, 3)
    _msg, _spec, _params, eng = build(txt, seed=5)
    x = np.random.default_rng(8).random((1, 3, 448, 448), dtype=np.float32)
    eng.host_array("data")[...] = x
    first = {k: v.copy() for k, v in eng.forward().items()}
    second = eng.forward()                                   # replay of the captured graph
    plain = eng.forward(use_graph=False)
    for k in first:
        assert np.array_equal(first[k], second[k]) and np.array_equal(first[k], plain[k]), k
    concat = eng.read_blob("conv4_3/conv5_3/concat").copy()
    eng.upload_inputs()
    eng.forward_resident(2)
    assert np.array_equal(eng.read_blob("conv4_3/conv5_3/concat"), concat)
    rows = eng.time_ops(2)                                   # every op launches alone on the engine's stream
    assert {"avepool", "deconv", "copy"} <= {r[0] for r in rows} and all(r[2] > 0 for r in rows)
    eng.close()
    monkeypatch.setenv("FCN_NO_GRAPH", "1")
    _msg, _spec, _params, eng2 = build(txt, seed=5)
    eng2.host_array("data")[...] = x
    out2 = eng2.forward()
    for k in first:
        assert np.array_equal(first[k], out2[k]), k
    eng2.close()


def test_forward_pipeline_of_f16_vgg_engines(gpu):
    from fcn_object_detector_amd.engine import ForwardPipeline
    msg, _spec, params, eng = build(models.vgg16_fcn_bbox_deploy(1, 96, 64, 4), seed=7)
    rng = np.random.default_rng(1)
    frames = [{"data": rng.random((1, 3, 96, 64), dtype=np.float32)} for _ in range(5)]
    want = []
    for f in frames:
        eng.host_array("data")[...] = f["data"]
        want.append({k: v.copy() for k, v in eng.forward().items()})
    pipe = ForwardPipeline(lambda: NetSpec(msg, "TEST"), params=params, device=0, depth=2, autotune=False, dtype="f16")
    got = pipe.map(frames)
    for g_, w_ in zip(got, want):
        for k in w_:
            assert np.array_equal(g_[k], w_[k]), k
    pipe.close()
    eng.close()


@pytest.mark.parametrize("cfg", [None, 0, 23])
def test_conv_float32_in_halves_out(gpu, monkeypatch, cfg):
    """FCN_CONV_OUT_F16 as conv1_1 of an f16 VGG engine uses it: float32 image (3 channels in 4-float pixels), float32 filters,
    3x3 / stride 1 / pad 1 -> 64 half channels with ReLU, in the default plan and two forced tile configurations; slack untouched."""
    if cfg is None:
        monkeypatch.delenv("FCN_CONV_CFG", raising=False)
    else:
        monkeypatch.setenv("FCN_CONV_CFG", str(cfg))
    n, h, w, cout, ycs, yo = 2, 61, 45, 64, 80, 8
    rng = np.random.default_rng(12)
    x = rng.random((n, 3, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, 3, 3, 3)) / np.sqrt(27)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) * 0.1
    want = R.relu(R.conv2d(x, wt, b, 1, 1))
    with Guards() as g:
        x4 = poisoned_nhwc(x, 4, 0)
        x4[..., 3] = 0.0                      # the pad channel of the image is multiplied (by a zero filter channel): it must be finite
        xd = g.put(x4, at_end=True, name="x")
        wd, bd = g.put(pack_ohwi(wt), name="w"), g.put(b, name="bias")
        yd = g.put(poisoned((n, h, w, ycs), dtype=np.float16), name="y")
        d = conv_desc(xd, wd, bd, yd, n, h, w, 4, 4, cout, 3, 1, 1, h, w, ycs, yo, L.CONV_OUT_F16 | L.CONV_RELU)
        L.call("fcn_conv2d_fwd_f32", C.byref(d), None)
        full = yd.read((n, h, w, ycs), np.float16)
    got = np.ascontiguousarray(full[..., yo:yo + cout].transpose(0, 3, 1, 2))
    assert slice_untouched(full, yo, cout)
    ref16 = want.astype(np.float16)
    ulp = np.abs(got.view(np.int16).astype(np.int32) - ref16.view(np.int16).astype(np.int32))
    print("OUT_F16 cfg %s: %.3g of the elements differ from the rounded oracle" % (cfg, (got != ref16).mean()))
    assert np.all((ulp <= 1) | (np.abs(got.astype(np.float32) - want) <= 2.0 ** -11 * np.abs(want) + 1e-6))


def test_what_the_f16_engine_still_refuses(gpu):
    """By name: a TRAIN net, and an Eltwise between a half blob and a float32 one (the two sides of a Sigmoid stay float32)."""
    tmsg = proto.parse_text(models.vgg16_fcn_bbox_train("m", "L", "unused", num_classes=3))
    with pytest.raises(NotImplementedError, match="inference only"):
        Engine(NetSpec(tmsg, "TRAIN"), {"data": (1, 3, 64, 64)}, device=0, autotune=False, dtype="f16")
    conv = ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: 8 kernel_size: 1 '
            'weight_filler { type: "xavier" } } }\n')
    txt = ('input: "data"\ninput_shape { dim: 1 dim: 3 dim: 8 dim: 8 }\n' + conv % ("a", "data", "a") + conv % ("b", "a", "b") + conv % ("c", "a", "c") +
           'layer { name: "sig" type: "Sigmoid" bottom: "c" top: "s" }\n'
           'layer { name: "mix" type: "Eltwise" bottom: "b" bottom: "s" top: "m" eltwise_param { operation: SUM } }\n' + conv % ("out", "m", "out"))
    msg = proto.parse_text(txt)
    with pytest.raises(NotImplementedError, match="Eltwise mix mixes half and float32"):
        Engine(NetSpec(msg, "TEST"), device=0, autotune=False, dtype="f16")
    eng = Engine(NetSpec(msg, "TEST"), device=0, autotune=False, dtype="f32")      # the float32 engine takes the same net
    eng.forward()
    eng.close()
