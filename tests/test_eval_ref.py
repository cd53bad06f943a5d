"""The numpy Accuracy reference on hand cases, NetSpec's shapes for the layer, and `caffe test`'s argument checks (no GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_eval64 as E
from conftest import PYCAFFE, ROOT
from fcn_object_detector_amd import proto
from fcn_object_detector_amd.netspec import NetSpec

CAFFE = os.path.join(ROOT, "fcn_object_detector_amd", "build", "tools", "caffe")


def px(*vectors):
    """Score vectors, one per pixel -> (1, C, 1, P)."""
    return np.asarray(vectors, np.float32).T[None, :, None, :]


def test_top1_and_ties_count_against_the_label():
    x = px([1, 3, 2], [5, 5, 1], [0, 0, 0], [2, 1, 0])
    lab = np.array([1, 0, 2, 0]).reshape(1, 1, 1, 4)
    ok, valid, ok_c, n_c = E.accuracy_counts(x, lab)
    # pixel 0: label is the strict maximum; pixel 1: tied with channel 1 -> wrong; pixel 2: tied with two -> wrong; pixel 3: right
    assert (ok, valid) == (2, 4)
    assert ok_c.tolist() == [1, 1, 0] and n_c.tolist() == [2, 1, 1]
    acc, per = E.accuracy(x, lab)
    assert acc == np.float32(0.5) and per.tolist() == [0.5, 1.0, 0.0]


def test_top_k_3():
    x = px([4, 3, 2, 1, 0], [4, 3, 2, 1, 0], [4, 3, 3, 3, 0])
    lab = np.array([2, 3, 3]).reshape(1, 1, 1, 3)
    # label 2 is third -> in the top 3; label 3 is fourth -> out; third pixel: 4, 3, 3 are >= the label's 3 (ties) -> three others -> out
    assert E.accuracy_counts(x, lab, top_k=3)[:2] == (1, 3)
    assert E.accuracy_counts(x, lab, top_k=1)[:2] == (0, 3)


def test_ignore_label_and_all_ignored():
    x = px([1, 0], [0, 1], [1, 0])
    lab = np.array([0, 255, 1]).reshape(1, 1, 1, 3)
    ok, valid, ok_c, n_c = E.accuracy_counts(x, lab, ignore_label=255)
    assert (ok, valid) == (1, 2) and n_c.tolist() == [1, 1] and ok_c.tolist() == [1, 0]
    acc, per = E.accuracy(x, np.full((1, 1, 1, 3), 255), ignore_label=255)
    assert acc == 0 and per.tolist() == [0.0, 0.0]


def test_out_of_range_label_is_valid_and_wrong():
    x = px([1, 0], [0, 1])
    for bad in (7, -1):
        ok, valid, ok_c, n_c = E.accuracy_counts(x, np.array([0, bad]).reshape(1, 1, 1, 2))
        assert (ok, valid) == (1, 2) and n_c.tolist() == [1, 0]
    # ... unless it is the ignore label
    assert E.accuracy_counts(x, np.array([0, 7]).reshape(1, 1, 1, 2), ignore_label=7)[:2] == (1, 1)


def test_running_sum_is_float32_in_call_order():
    rng = np.random.default_rng(0)
    xs = [rng.standard_normal(1000).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 4)) for _ in range(5)]
    acc = np.zeros(1000, np.float32)
    for x in xs:
        acc += x
    assert np.array_equal(E.running_sum(xs).view(np.uint32), acc.view(np.uint32))
    assert np.array_equal(E.test_mean(xs).view(np.uint32), (acc / np.float32(5)).view(np.uint32))


NET = """
input: "score" input_shape { dim: 2 dim: 5 dim: 3 dim: 4 }
input: "label" input_shape { dim: 2 dim: 1 dim: 3 dim: 4 }
layer { name: "acc" type: "Accuracy" bottom: "score" bottom: "label" top: "accuracy" %s %s }
"""


def test_netspec_infers_accuracy_shapes():
    spec = NetSpec(proto.parse_text(NET % ('top: "per_class"', "accuracy_param { top_k: 2 ignore_label: 255 }")), "TEST")
    shapes = spec.infer()
    assert shapes["accuracy"] == () and shapes["per_class"] == (5,)
    assert spec.output_blobs() == ["accuracy", "per_class"] and spec.param_layers() == []
    spec = NetSpec(proto.parse_text(NET % ("", "")), "TEST")
    assert spec.infer()["accuracy"] == () and "per_class" not in spec.blob_shapes


def test_netspec_refuses_accuracy_over_another_axis():
    with pytest.raises(NotImplementedError, match="acc"):
        NetSpec(proto.parse_text(NET % ("", "accuracy_param { axis: 2 }")), "TEST").infer()
    with pytest.raises(ValueError, match="top_k"):
        NetSpec(proto.parse_text(NET % ("", "accuracy_param { top_k: 6 }")), "TEST").infer()


def run_tool(*args):
    env = dict(os.environ, PYTHONPATH=PYCAFFE + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, CAFFE] + list(args), capture_output=True, text=True, timeout=120, env=env)


def test_caffe_test_needs_model_and_weights(tmp_path):
    r = run_tool("test")
    assert r.returncode == 1 and "Need a model definition to score." in r.stderr
    model = tmp_path / "net.prototxt"
    model.write_text(NET % ("", ""))
    r = run_tool("test", "--model=%s" % model)
    assert r.returncode == 1 and "Need model weights to score." in r.stderr
    r = run_tool("bogus")
    assert r.returncode == 1 and "caffe test --model=" in r.stderr
