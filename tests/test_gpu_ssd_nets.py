"""MobileNet-SSD (models.mobilenet_ssd at width_div 8, 96 x 96, batch 2) and an SSD300-VGG fragment (models.ssd300_vgg at width_div 16,
32 x 32, batch 2, the conv4_3_norm, fc7 and conv6_2 heads) through caffe.Net from a prototxt and a caffemodel, -m gpu, against torch float64 for
the body and tests/ref_ssd64.py for the head (tests/ssd_net_ref.py; tests/test_ssd_ref.py asserts the decision margin of both nets
without a GPU).

Blobs are held to the project's rel_err < 1e-4; detection_out to the same count, the same (image, label) per row in the same order, and
score and corners within 1e-5 absolute of float64, as in tests/test_gpu_guarded_ssd.py (the error of the tail's own inputs - the
net's scores and box codes - is printed beside it)."""
import sys

import numpy as np
import pytest

import ssd_cases
import ssd_net_ref as N
from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto

pytestmark = pytest.mark.gpu
HEAD_BLOBS = ["mbox_loc", "mbox_conf", "mbox_priorbox", "mbox_conf_softmax", "mbox_conf_reshape", "mbox_conf_flatten"]
BODY = {"mobilenet_ssd": ["conv0", "conv5/dw", "conv11", "conv13", "conv14_2", "conv17_2", "conv11_mbox_loc", "conv13_mbox_conf", "conv17_2_mbox_conf"],
        "ssd300_vgg": ["conv1_1", "conv4_3", "conv4_3_norm", "fc6", "fc7", "conv6_2", "conv4_3_norm_mbox_loc", "fc7_mbox_conf", "conv6_2_mbox_conf"]}


def _caffe():
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    return caffe


@pytest.fixture(scope="module", params=["mobilenet_ssd", "ssd300_vgg"])
def case(request, tmp_path_factory):
    """One net, built once through caffe.Net, one forward, and its float64 reference - shared by the tests below and left unchanged."""
    from fcn_object_detector_amd import lib as L
    L.load()
    caffe = _caffe()
    name = request.param
    text, spec, params, x = N.build(name)
    d = tmp_path_factory.mktemp(name)
    deploy, weights = d / "deploy.prototxt", d / "w.caffemodel"
    deploy.write_text(text)
    proto.write_caffemodel(str(weights), [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    net = caffe.Net(str(deploy), str(weights), caffe.TEST)
    net.blobs["data"].data[...] = x
    out = net.forward()
    B, margin, count = N.reference(name, spec, params, x)
    yield dict(name=name, net=net, out={k: v.copy() for k, v in out.items()}, ref=B, margin=margin, count=count, spec=spec, deploy=str(deploy),
               weights=str(weights), x=x)
    net._engine.close()


def test_body_and_head_blobs(gpu, case):
    net, B = case["net"], case["ref"]
    for nm in BODY[case["name"]] + HEAD_BLOBS:
        got = net.blobs[nm].data
        assert got.shape == B[nm].shape == tuple(net.blobs[nm].shape), nm
        err = rel_err(got, B[nm])
        print("BLOB %s %s %.3g" % (case["name"], nm, err))
        assert err < 1e-4, nm
    assert np.max(np.abs(net.blobs["mbox_priorbox"].data - B["mbox_priorbox"])) < 1e-6


def test_blob_shapes_are_caffes(gpu, case):
    net, spec = case["net"], case["spec"]
    for l in spec.layers:
        if l.type in ("Permute", "Flatten", "Reshape", "PriorBox"):
            top = l.tops[0]
            assert tuple(net.blobs[top].shape) == tuple(net.blobs[top].data.shape) == tuple(case["ref"][top].shape), top
            assert rel_err(net.blobs[top].data, case["ref"][top]) < 1e-4, top
    feat = "conv11" if case["name"] == "mobilenet_ssd" else "fc7"
    n, c, h, w = net.blobs[feat + "_mbox_conf"].shape
    assert net.blobs[feat + "_mbox_conf_perm"].shape == (n, h, w, c) and net.blobs[feat + "_mbox_conf_flat"].shape == (n, h * w * c)
    p = net.blobs["mbox_loc"].shape[1] // 4
    assert net.blobs["mbox_conf_reshape"].shape == (n, p, 21) and net.blobs["mbox_priorbox"].shape == (1, 2, p * 4)


def test_detection_out(gpu, case):
    net, want, count = case["net"], case["ref"]["detection_out"], case["count"]
    assert case["margin"] >= ssd_cases.MARGIN and count > 0
    got = case["out"]["detection_out"]
    assert got.shape == (1, 1, count, 7) == tuple(net.blobs["detection_out"].shape) == net.blobs["detection_out"].data.shape
    assert np.array_equal(net.blobs["detection_out"].data, got)
    rows = got[0, 0].astype(np.float64)
    assert np.array_equal(rows[:, :2], want[:, :2]), "image / label of the rows, in order"
    # (printed only: what reaches the tail is the net's - scores off by the softmax blob's error, corners by the decoded loc's)
    B = case["ref"]
    own = max(rel_err(net.blobs["mbox_conf_softmax"].data, B["mbox_conf_softmax"]) * float(np.abs(B["mbox_conf_softmax"]).max()),
              rel_err(net.blobs["mbox_loc"].data, B["mbox_loc"]) * float(np.abs(B["mbox_loc"]).max()) * 0.2)
    err = float(np.max(np.abs(rows[:, 2:] - want[:, 2:])))
    print("DETOUT %s rows %d worst |error| %.3g (inputs of the tail off by %.3g) margin %.3g" % (case["name"], count, err, own, case["margin"]))
    assert err <= 1e-5
    # the engine's ops: the two gathers, the row softmax, one detection tail (and Normalize in the VGG net)
    kinds = [op.kind for op in net._engine.ops]
    assert kinds.count("ssd_gather") == 2 and kinds.count("detection_output") == 1 and kinds.count("softmax") == 1 and "copy" not in kinds
    assert kinds.count("normalize") == (1 if case["name"] == "ssd300_vgg" else 0)


def test_replay_and_eager_give_the_same_bytes(gpu, case, monkeypatch):
    """Two forwards through the captured graph and two with FCN_NO_GRAPH=1 (plain launches) on one net - one plan, as tests/test_gpu_net.py
    compares them: two nets may be tuned to different tiles, whose sums round differently."""
    net, outs = case["net"], []
    for no_graph in ("0", "1"):
        monkeypatch.setenv("FCN_NO_GRAPH", no_graph)
        for _ in range(2):
            net.blobs["data"].data[...] = case["x"]
            outs.append(net.forward()["detection_out"].copy())
    assert net._engine.graph_io is not None
    assert all(o.tobytes() == case["out"]["detection_out"].tobytes() for o in outs)


def test_an_image_without_detections_gives_caffes_block(gpu, case):
    """Quiet conf heads everywhere (zero banks, the background bias alone - no hot entry): every score is e^-8 / (1 + 20 e^-8) = 3.3e-4,
    K == 0, and the top is the (1, 1, N, 7) block of -1 with the image index in column 0."""
    caffe = _caffe()
    net = caffe.Net(case["deploy"], case["weights"], caffe.TEST)
    try:
        for lname in net.params:
            if lname.endswith("_mbox_conf"):
                net.params[lname][0].data[...] = 0.0
                bias = net.params[lname][1].data
                bias[...] = 0.0
                bias.reshape(-1, 21)[:, 0] = N.BACKGROUND_BIAS
        net.blobs["data"].data[...] = case["x"]
        out = net.forward()["detection_out"]
        assert out.shape == (1, 1, 2, 7) == tuple(net.blobs["detection_out"].shape)
        assert out[0, 0].tolist() == [[0.0] + [-1.0] * 6, [1.0] + [-1.0] * 6]
    finally:
        net._engine.close()


def test_the_training_writers_refuse(gpu):
    for fn in (models.mobilenet_ssd, models.ssd300_vgg):
        for phase in ("TRAIN", "TEST"):
            with pytest.raises(NotImplementedError, match="MultiBoxLoss"):
                fn(phase)


def test_the_half_float_engine_refuses_by_its_wording(gpu, case):
    caffe = _caffe()
    with pytest.raises(NotImplementedError, match=r"f16 engine: layer type \w+ \(\S+\) has no half-float kernel"):
        caffe.Net(case["deploy"], case["weights"], caffe.TEST, dtype="f16")
