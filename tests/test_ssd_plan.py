"""The SSD head as the forward planner lays it out - without a GPU.

As tests/test_dilation_plan.py: Engine methods run on the stub engine of tests/plan_stub.py with DeviceBuffer replaced by a counter of addresses and the library
by one whose entry points return 0 (size queries: 64).  Checked: one ssd_gather op per Concat with the right heads and columns and no copy
op, nothing for Permute / Flatten / Reshape / PriorBox, the prior constants against the float64 reference, the order of the ops, the
capacity of detection_out, and the TRAIN-phase refusal."""
import ctypes as C

import numpy as np
import pytest

import ref_ssd64 as R
from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import models, ssd
from plan_stub import engine_factory


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, backward=False, depthwise=True)


def ssd_ops(e):
    return [(op.kind, op.name) for t in e.tasks if isinstance(t, E.OpTask) for op in t.ops if op.kind in ("ssd_gather", "normalize", "softmax", "detection_output", "copy")]


def heads_of(e, kind):
    arr = next(k for k in e._keep if isinstance(k, C.Array) and k._type_ is L.SsdHead and k[0].src == e.blobs["conv4_3_norm_mbox_%s" % kind].buf.ptr)
    return [(h.src, h.pixels, h.C, h.cstride, h.coffset, h.dst_col) for h in arr]


def test_ssd300_fragment_plan(stub):
    e = stub(models.ssd300_vgg(width_div=16, size=64, batch=2, heads=2))
    B = e.blobs
    # two gathers, Normalize in front, the row softmax and the detection tail behind; no copy op for the Concats, nothing else of the head
    assert ssd_ops(e) == [("normalize", "conv4_3_norm"), ("ssd_gather", "mbox_loc:conv4_3_norm_mbox_loc+fc7_mbox_loc"),
                          ("ssd_gather", "mbox_conf:conv4_3_norm_mbox_conf+fc7_mbox_conf"), ("softmax", "mbox_conf_softmax"),
                          ("detection_output", "detection_out")]
    emitting = {t.layer.name for t in e.tasks if isinstance(t, E.OpTask) and t.ops}
    assert not emitting & {l.name for l in e.spec.layers if l.type in ("Permute", "Flatten", "Reshape", "PriorBox")} and "mbox_priorbox" not in emitting
    # the heads: 8 x 8 cells of 4 priors, 4 x 4 cells of 6; loc C = 16 / 24 (cstride as is), conf C = 84 / 126 (cstride 84 / 128)
    assert heads_of(e, "loc") == [(B["conv4_3_norm_mbox_loc"].buf.ptr, 64, 16, 16, 0, 0), (B["fc7_mbox_loc"].buf.ptr, 16, 24, 24, 0, 1024)]
    assert heads_of(e, "conf") == [(B["conv4_3_norm_mbox_conf"].buf.ptr, 64, 84, 84, 0, 0), (B["fc7_mbox_conf"].buf.ptr, 16, 126, 128, 0, 5376)]
    # the Flatten tops are windows of the Concat top, the Permute tops own nothing, Reshape / Flatten of the scores share one buffer each
    f = B["fc7_mbox_conf_flat"]
    assert f.buf is B["mbox_conf"].buf and (f.coffset, f.cstride, f.shape) == (5376, 7392, (2, 2016)) and "fc7_mbox_conf_perm" not in B
    assert B["mbox_conf_reshape"].buf is B["mbox_conf"].buf and B["mbox_conf_flatten"].buf is B["mbox_conf_softmax"].buf
    assert B["mbox_conf_softmax"].buf is not B["mbox_conf"].buf and B["mbox_conf_softmax"].cstride == 7392
    gather_calls = [a for n, a in e.fake.calls if n == "fcn_ssd_gather_f32"]
    assert gather_calls == []                                                      # (planned, not launched)
    for t in e.tasks:
        if isinstance(t, E.OpTask):
            for op in t.ops:
                if op.kind in ("ssd_gather", "softmax", "detection_output", "normalize"):
                    op.run(None)
    g = [a for n, a in e.fake.calls if n == "fcn_ssd_gather_f32"]
    assert [(a[1], a[2], a[3], a[4], a[5]) for a in g] == [(2, 2, B["mbox_loc"].buf.ptr, 1408, 1408), (2, 2, B["mbox_conf"].buf.ptr, 7392, 7392)]
    sm = [a for n, a in e.fake.calls if n == "fcn_softmax_fwd_f32"]
    x, y = B["mbox_conf"].buf.ptr, B["mbox_conf_softmax"].buf.ptr
    assert [a[:6] for a in sm] == [(x, y, 352, 21, 21, 21), (x + 4 * 7392, y + 4 * 7392, 352, 21, 21, 21)]      # one launch per image row
    # order: every task waits for what it reads
    lv = dict(zip([t.layer.name for t in e.tasks], E.task_levels(e.tasks)))
    assert lv["conv4_3_norm"] < lv["conv4_3_norm_mbox_loc"] < lv["mbox_loc"] < lv["detection_out"]
    assert lv["fc7_mbox_conf"] < lv["mbox_conf"] < lv["mbox_conf_softmax"] < lv["detection_out"]
    # detection_out: 2 images x keep_top_k 200 rows of capacity, the count behind them
    par = next(k for k in e._keep if isinstance(k, L.DetOutParams))
    assert (par.N, par.P, par.num_classes, par.background, par.code_type, par.top_k, par.keep_top_k, par.capacity) == (2, 352, 21, 0, 2, 400, 200, 400)
    assert (par.loc_rstride, par.conf_rstride) == (1408, 7392) and abs(par.conf_threshold - 0.01) < 1e-9 and abs(par.nms_threshold - 0.45) < 1e-7
    d = [a for n, a in e.fake.calls if n == "fcn_detection_output_f32"][0]
    out = B["detection_out"]
    assert out.buf.nbytes == 4 * (400 * 7 + 4) and out.nchw is None and e.detections == {"detection_out": 400}
    assert (d[0], d[1], d[2], d[4], d[5]) == (B["mbox_loc"].buf.ptr, y, B["mbox_priorbox"].buf.ptr, out.buf.ptr, out.buf.ptr + 4 * 7 * 400)
    assert e.blob_shape("detection_out") == (1, 1, 400, 7)                          # before any forward: the capacity
    nm = [a for n, a in e.fake.calls if n == "fcn_normalize_fwd_f32"][0]
    assert nm[3:10] == (2 * 64, 32, 32, 0, 32, 0, 0) and abs(nm[10] - 1e-10) < 1e-16 and nm[2] == e.params_dev["conv4_3_norm"][0].ptr


def test_prior_constants_equal_the_reference(stub):
    e = stub(models.ssd300_vgg(width_div=16, size=64, batch=2, heads=2))
    k = 64 / 300.0
    a = R.prior_box(8, 8, 64, 64, [30 * k], [60 * k], [2.0], variance=(0.1, 0.1, 0.2, 0.2))
    b = R.prior_box(4, 4, 64, 64, [60 * k], [111 * k], [2.0, 3.0], variance=(0.1, 0.1, 0.2, 0.2))
    want = np.concatenate([a, b], axis=2)
    got = e.prior_consts["mbox_priorbox"]
    assert got.shape == (1, 2, 1408) and got.dtype == np.float32 and np.max(np.abs(got - want)) < 1e-6
    assert np.max(np.abs(e.prior_consts["fc7_mbox_priorbox"] - b)) < 1e-6
    # uploaded once, as they lie: corners, then variances
    assert e.copied[e.blobs["mbox_priorbox"].buf.ptr] == got.tobytes() and e.read_blob("mbox_priorbox") is got
    # the published steps at 300: 8 and 16
    full = stub(models.ssd300_vgg(width_div=32, heads=2))
    a = R.prior_box(38, 38, 300, 300, [30.0], [60.0], [2.0], variance=(0.1, 0.1, 0.2, 0.2), step=8)
    b = R.prior_box(19, 19, 300, 300, [60.0], [111.0], [2.0, 3.0], variance=(0.1, 0.1, 0.2, 0.2), step=16)
    assert np.max(np.abs(full.prior_consts["mbox_priorbox"] - np.concatenate([a, b], axis=2))) < 1e-6


def many_heads(n, concat=True):
    s = ['input: "data" input_shape { dim: 2 dim: 3 dim: 6 dim: 5 }']
    for i in range(n):
        s.append('layer { name: "h%d" type: "Convolution" bottom: "data" top: "h%d" convolution_param { num_output: %d kernel_size: 1 } }' % (i, i, 3 + i % 3))
        s.append('layer { name: "p%d" type: "Permute" bottom: "h%d" top: "p%d" permute_param { order: 0 order: 2 order: 3 order: 1 } }' % (i, i, i))
        s.append('layer { name: "f%d" type: "Flatten" bottom: "p%d" top: "f%d" }' % (i, i, i))
    if concat:
        s.append('layer { name: "cat" type: "Concat" %s top: "cat" }' % " ".join('bottom: "f%d"' % i for i in range(n)))
    return "\n".join(s)


def test_more_heads_than_a_launch_takes_and_a_lone_flatten(stub):
    e = stub(many_heads(17))
    assert [(k, n.split(":")[0], n.count("+") + 1) for k, n in ssd_ops(e)] == [("ssd_gather", "cat", 16), ("ssd_gather", "cat", 1)]
    last = next(k for k in e._keep if isinstance(k, C.Array) and len(k) == 1)
    assert (last[0].C, last[0].cstride, last[0].dst_col) == (4, 4, 30 * sum(3 + i % 3 for i in range(16)))
    lone = stub(many_heads(1, concat=False))
    assert ssd_ops(lone) == [("ssd_gather", "f0:h0")] and lone.blobs["f0"].buf.nbytes == 2 * 92 * 4      # 90 columns in rows of 92


def test_a_train_net_refuses_the_head_by_layer_name(stub):
    text = many_heads(1, concat=False) + '\ninput: "t" input_shape { dim: 2 dim: 90 }\nlayer { name: "loss" type: "EuclideanLoss" bottom: "f0" bottom: "t" top: "loss" }'
    with pytest.raises(NotImplementedError, match="layer p0: Permute below a layer that learns in a TRAIN-phase net"):
        stub(text, phase="TRAIN")


def test_detection_rows_are_composed_on_the_host():
    raw = np.zeros(3 * 7 + 4, np.float32)
    raw[:14] = np.arange(14)
    out = ssd.compose_detections(raw, 2, 3)
    assert out.shape == (1, 1, 2, 7) and out[0, 0, 1].tolist() == list(range(7, 14))
    none = ssd.compose_detections(raw, 0, 3)
    assert none.shape == (1, 1, 3, 7) and none[0, 0].tolist() == [[i, -1, -1, -1, -1, -1, -1] for i in range(3)]


SCORES = """input: "d" input_shape { dim: 2 dim: 3 dim: 4 dim: 4 }
layer { name: "c" type: "Convolution" bottom: "d" top: "c" convolution_param { num_output: 18 kernel_size: 1 } }
layer { name: "p" type: "Permute" bottom: "c" top: "p" permute_param { order: 0 order: 2 order: 3 order: 1 } }
layer { name: "s" type: "Flatten" bottom: "p" top: "s" }
layer { name: "rs" type: "Reshape" bottom: "s" top: "rs" reshape_param { shape { dim: 0 dim: -1 dim: 3 } } }
layer { name: "sm" type: "Softmax" bottom: "rs" top: "sm" %s }
"""


def test_softmax_of_a_3d_blob_runs_over_its_last_axis_only(stub):
    """An (N, P, C) blob lies as rows of P * C floats: axis 2 (or -1) is the row softmax; the default axis 1 - Caffe: over P for each C -
    and axis 0 keep the engine's refusal instead of normalising over the whole row."""
    for axis in ("softmax_param { axis: 2 }", "softmax_param { axis: -1 }"):
        assert ("softmax", "sm") in ssd_ops(stub(SCORES % axis))
    for axis in ("", "softmax_param { axis: 1 }", "softmax_param { axis: 0 }"):
        with pytest.raises(NotImplementedError, match=r"Softmax over an axis other than channels \(layer sm\)"):
            stub(SCORES % axis)
