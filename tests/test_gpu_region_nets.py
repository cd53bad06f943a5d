"""A Fast-R-CNN-style fragment (conv, ROIPooling of Input-fed rois, InnerProduct, Softmax) and the R-FCN deploy net
(models.rfcn_resnet(50, width_div=8, size=96, classes=5), pre / post_nms_topn 60 / 12) through caffe.Net from a prototxt and a caffemodel,
-m gpu, against torch float64 for the body and tests/ref_region64.py for the region stage (tests/region_net_ref.py; tests/test_region_ref.py
asserts the decision margin of both nets without a GPU).

Blobs are held to the project's rel_err < 1e-4, as tests/test_gpu_ssd_nets.py holds them; rois to the reference's count and order, corners
within the kernel test's 32 ulps of the image extent plus the error of the RPN's own outputs (printed)."""
import sys

import numpy as np
import pytest

import region_cases as RC
import region_net_ref as N
from conftest import PYCAFFE, rel_err
from fcn_object_detector_amd import models, proto

pytestmark = pytest.mark.gpu
BLOBS = {"fast": ["conv", "roi_pool", "fc", "prob"],
         "rfcn": ["conv1", "res4f", "res5c", "rpn_cls_score", "rpn_bbox_pred", "rpn_cls_score_reshape", "rpn_cls_prob", "rpn_cls_prob_reshape", "rfcn_cls",
                  "rfcn_bbox", "psroipooled_cls_rois", "psroipooled_loc_rois", "cls_score", "cls_prob", "bbox_pred"]}


def _caffe():
    if PYCAFFE not in sys.path:
        sys.path.insert(0, PYCAFFE)
    import caffe
    return caffe


def _feed(net, inputs):
    for k, v in inputs.items():
        net.blobs[k].data[...] = v


@pytest.fixture(scope="module", params=["fast", "rfcn"])
def case(request, tmp_path_factory):
    """One net, built once through caffe.Net, one forward, and its float64 reference - shared by the tests below and left unchanged."""
    from fcn_object_detector_amd import lib as L
    L.load()
    caffe = _caffe()
    name = request.param
    text, spec, params, inputs = N.build(name)
    d = tmp_path_factory.mktemp(name)
    deploy, weights = d / "deploy.prototxt", d / "w.caffemodel"
    deploy.write_text(text)
    proto.write_caffemodel(str(weights), [(l.name, l.type, params[l.name]) for l in spec.param_layers()])
    net = caffe.Net(str(deploy), str(weights), caffe.TEST)
    _feed(net, inputs)
    out = net.forward()
    B, margin, count, prop = N.reference(name, spec, params, inputs)
    yield dict(name=name, net=net, out={k: v.copy() for k, v in out.items()}, ref=B, margin=margin, count=count, prop=prop, spec=spec,
               deploy=str(deploy), weights=str(weights), inputs=inputs)
    net._engine.close()


def test_rois_count_and_order(gpu, case):
    net, B, count = case["net"], case["ref"], case["count"]
    assert case["margin"] >= RC.MARGIN
    if case["name"] == "fast":      # rois through an Input layer: all R rows are real, nothing is cut
        assert net.blobs["rois"].shape == (8, 5) and net.blobs["roi_pool"].shape == (8, 10, 3, 2) and net._engine.roi_counts == {}
        return
    assert 0 < count < 12 and case["prop"]["suppressed"] > 0
    rois = net.blobs["rois"].data
    assert net.blobs["rois"].shape == (count, 5) == rois.shape and net.blobs["rois"].shape[0] == count
    for nm in ("psroipooled_cls_rois", "cls_score", "cls_prob", "bbox_pred"):
        assert net.blobs[nm].shape[0] == count == net.blobs[nm].data.shape[0], nm
    assert np.all(rois[:, 0] == 0)
    want = B["rois"]
    # what reaches Proposal is the net's: corners off by the error of the RPN's box deltas times the anchors' extent, besides the kernel's own
    own = rel_err(net.blobs["rpn_bbox_pred"].data, B["rpn_bbox_pred"]) * float(np.abs(B["rpn_bbox_pred"]).max()) * 192.0 * 4
    err = float(np.max(np.abs(rois[:, 1:].astype(np.float64) - want[:, 1:])))
    limit = 32 * float(np.spacing(np.float32(96.0)))
    print("ROIS rfcn rows %d worst |error| %.3g (limit %.3g + inputs of the layer off by %.3g) margin %.3g" % (count, err, limit, own, case["margin"]))
    assert err <= limit + own
    far = np.abs(rois[:, None, 1:].astype(np.float64) - want[None, :, 1:]).max(axis=2)
    assert np.array_equal(np.argmin(far, axis=1), np.arange(count)), "the rows' order"
    # the rows behind the count are zeros on the device: the poolings run over all post_nms_topn rows
    eng = net._engine
    full = eng.blobs["rois"]
    raw = np.empty((12, full.cstride), np.float32)
    from fcn_object_detector_amd import lib as L
    L.call("fcn_memcpy_d2h_async", raw.ctypes.data, full.buf.ptr, raw.nbytes, None)
    L.call("fcn_device_sync")
    assert np.all(raw[count:] == 0) and np.all(raw[:, 5:] == 0)
    kinds = [op.kind for op in eng.ops]
    assert kinds.count("pair_softmax") == 1 and kinds.count("proposal") == 1 and kinds.count("psroi_pool") == 2


def test_blobs(gpu, case):
    net, B = case["net"], case["ref"]
    for nm in BLOBS[case["name"]]:
        got = net.blobs[nm].data
        assert got.shape == B[nm].shape == tuple(net.blobs[nm].shape), nm
        err = rel_err(got, B[nm])
        print("BLOB %s %s %.3g" % (case["name"], nm, err))
        assert err < 1e-4, nm
    for nm in N.OUTPUTS[case["name"]]:
        assert case["out"][nm].shape == B[nm].shape and rel_err(case["out"][nm], B[nm]) < 1e-4, nm
    if case["name"] == "rfcn":
        assert np.allclose(net.blobs["cls_prob"].data.sum(axis=1), 1.0, atol=1e-5)


def test_replay_and_eager_give_the_same_bytes(gpu, case, monkeypatch):
    """Two forwards through the captured graph and two with FCN_NO_GRAPH=1 (plain launches) on one net, as tests/test_gpu_ssd_nets.py
    compares them."""
    net, outs = case["net"], []
    for no_graph in ("0", "1"):
        monkeypatch.setenv("FCN_NO_GRAPH", no_graph)
        for _ in range(2):
            _feed(net, case["inputs"])
            o = net.forward()
            outs.append(b"".join(o[k].tobytes() for k in N.OUTPUTS[case["name"]]) + net.blobs["rois"].data.tobytes())
    assert net._engine.graph_io is not None
    first = b"".join(case["out"][k].tobytes() for k in N.OUTPUTS[case["name"]])
    assert all(o.startswith(first) and o == outs[0] for o in outs)


def test_the_training_writer_refuses(gpu):
    for phase in ("TRAIN", "TEST"):
        with pytest.raises(NotImplementedError, match="AnchorTarget / ProposalTarget"):
            models.rfcn_resnet(phase)


def test_the_half_float_engine_refuses_by_its_wording(gpu, case):
    caffe = _caffe()
    with pytest.raises(NotImplementedError, match=r"f16 engine: layer type \w+ \(\S+\) has no half-float kernel"):
        caffe.Net(case["deploy"], case["weights"], caffe.TEST, dtype="f16")
