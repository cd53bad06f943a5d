"""Solver test nets on the device (-m gpu): weight sharing by aliasing the flat parameter buffer, the test schedule and its values
against a standalone TEST engine, the bundled data layer in both phases, the Accuracy layer inside a net, and `caffe test`.

The schedule tests use a data layer of their own, written into tmp_path: batch k is a function of (seed, k) alone - the bundled layer
draws from Python's global `random`, so a test pass would move the training stream (as it does under Caffe)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_eval64 as E
from conftest import PYCAFFE, ROOT
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.engine import Engine
from fcn_object_detector_amd.netspec import NetSpec, fill_params
from fcn_object_detector_amd.solver import Solver
from fcn_object_detector_amd.train import SolverParams, TrainEngine

pytestmark = pytest.mark.gpu

CAFFE = os.path.join(ROOT, "fcn_object_detector_amd", "build", "tools", "caffe")
MODULE = "testnet_counting_layer"
LAYER_SOURCE = '''
import numpy as np

TOPS = ("data", "coverage-label", "bbox-label", "size-block", "obj-block", "coverage-block")


def parse(param_str):
    w, h, stride, classes, batch, seed = (int(v) for v in param_str.split(","))
    return dict(w=w, h=h, stride=stride, classes=classes, batch=batch, seed=seed)


def batch(cfg, k):
    """Batch k of a layer with configuration cfg: a function of (seed, k) alone."""
    rng = np.random.default_rng(1000 * cfg["seed"] + k)
    n, c, gy, gx = cfg["batch"], cfg["classes"], cfg["h"] // cfg["stride"], cfg["w"] // cfg["stride"]
    cov = (rng.random((n, c, gy, gx)) < 0.25).astype(np.float32)
    rep = np.repeat(cov, 4, axis=1)
    return {"data": rng.random((n, 3, cfg["h"], cfg["w"]), dtype=np.float32),
            "coverage-label": cov,
            "bbox-label": (rng.standard_normal((n, 4 * c, gy, gx)) * 20).astype(np.float32) * rep,
            "size-block": np.full((n, 4 * c, gy, gx), 1.0 / cfg["w"], np.float32),
            "obj-block": rep.copy(),
            "coverage-block": rep.copy()}


class CountingLayer(object):
    def setup(self, bottom, top):
        self.cfg = parse(self.param_str)
        self.k = 0

    def reshape(self, bottom, top):
        for t, (name, a) in zip(top, batch(self.cfg, 0).items()):
            t.reshape(*a.shape)

    def forward(self, bottom, top):
        b = batch(self.cfg, self.k)
        for t, name in zip(top, TOPS):
            t.data[...] = b[name]
        self.k += 1

    def backward(self, top, propagate_down, bottom):
        pass
'''
TRAIN_CFG, TEST_CFG = "64,64,16,2,2,1", "96,64,16,2,1,2"      # W, H, stride, classes, batch, seed: TEST geometry differs from TRAIN


@pytest.fixture
def layer_module(tmp_path):
    (tmp_path / (MODULE + ".py")).write_text(LAYER_SOURCE)
    sys.path.insert(0, str(tmp_path))
    sys.modules.pop(MODULE, None)
    mod = __import__(MODULE)
    yield mod
    sys.path.remove(str(tmp_path))
    sys.modules.pop(MODULE, None)


def write_job(tmp_path, extra="", test=True, max_iter=4, classes=2):
    net = tmp_path / "train_val.prototxt"
    net.write_text(models.googlenet_detectnet_train(MODULE, "CountingLayer", TRAIN_CFG, num_classes=classes, test_param_str=TEST_CFG))
    solver = tmp_path / ("solver_test.prototxt" if test else "solver_plain.prototxt")
    solver.write_text('net: "%s"\nbase_lr: 1e-4\nmomentum: 0.9\nweight_decay: 1e-6\nlr_policy: "fixed"\ndisplay: 1\nmax_iter: %d\n'
                      'snapshot: 2\nsnapshot_prefix: "%s"\n%s%s'
                      % (net, max_iter, tmp_path / ("snap" if test else "plain"), "test_iter: 3\ntest_interval: 2\n" if test else "", extra))
    return str(solver), str(net)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_spec(net_file, mod, cfg=TEST_CFG):
    msg = proto.parse_file(net_file)
    shapes = {k: v.shape for k, v in mod.batch(mod.parse(cfg), 0).items()}
    spec = NetSpec(msg, "TEST")
    spec.infer(shapes)
    return spec, shapes


test_spec.__test__ = False


def forward_on(eng, batch):
    for k, v in batch.items():
        eng.host_array(k)[...] = v
    return {k: v.copy() for k, v in eng.forward().items()}


# ---- sharing ----------------------------------------------------------------------------------------------------------------------
def test_shared_parameters_alias_the_training_buffer(gpu, tmp_path, layer_module):
    mod = layer_module
    job, net_file = write_job(tmp_path, test=False)
    s = Solver(job, device=0, log=None, autotune=False)
    spec, shapes = test_spec(net_file, mod)
    te = Engine(spec, shapes, None, device=0, autotune=False, share_params=s.engine)
    assert te.shared_layers == {l.name for l in spec.param_layers()} and te.param_count == 0
    for l in spec.param_layers():
        for mine, theirs in zip(te.params_dev[l.name], s.engine.params_dev[l.name]):
            assert mine.ptr == theirs.ptr and mine.nbytes == theirs.nbytes
            assert s.engine.param_flat.ptr <= mine.ptr and mine.ptr + mine.nbytes <= s.engine.param_flat.ptr + s.engine.param_flat.nbytes
    fixed = mod.batch(mod.parse(TEST_CFG), 77)
    s.step(3)
    a = forward_on(te, fixed)
    spec2, _ = test_spec(net_file, mod)
    fresh = Engine(spec2, shapes, s.engine.download_params(), device=0, autotune=False)
    b = forward_on(fresh, fixed)
    assert set(a) == set(b) == {"loss_bbox", "loss_coverage"}
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    got = te.read_param("conv1/7x7_s2", 0)
    assert np.array_equal(bits(got), bits(s.engine.download_params()["conv1/7x7_s2"][0]))
    s.step(1)      # nothing is called on the test engine: the next forward simply reads the moved weights
    a4 = forward_on(te, fixed)
    assert any(not np.array_equal(bits(a4[k]), bits(a[k])) for k in a)
    with pytest.raises(RuntimeError, match="cvg/classifier"):
        te.set_params("cvg/classifier", s.engine.params_host["cvg/classifier"])
    # the half-float engine packs its weights differently: refused
    spec3, _ = test_spec(net_file, mod)
    with pytest.raises(NotImplementedError, match="share_params"):
        Engine(spec3, shapes, None, device=0, autotune=False, dtype="f16", share_params=s.engine)
    # closing in either order: the sharing engine first ...
    te.close()
    fresh.close()
    # ... or the owner first - the storage lives as long as anyone reads it
    spec4, _ = test_spec(net_file, mod)
    te2 = Engine(spec4, shapes, None, device=0, autotune=False, share_params=s.engine)
    s.close()
    a5 = forward_on(te2, fixed)
    for k in a4:
        assert np.array_equal(bits(a5[k]), bits(a4[k])), k
    te2.close()


def test_sharing_refuses_a_shape_mismatch_and_keeps_foreign_layers(gpu, tmp_path, layer_module):
    mod = layer_module
    job, net_file = write_job(tmp_path, test=False)
    s = Solver(job, device=0, log=None, autotune=False)
    other = tmp_path / "three_classes.prototxt"
    other.write_text(models.googlenet_detectnet_train(MODULE, "CountingLayer", "64,64,16,3,2,1", num_classes=3))
    spec, shapes = test_spec(str(other), mod, "64,64,16,3,2,1")
    with pytest.raises(ValueError, match="cvg/classifier"):
        Engine(spec, shapes, None, device=0, autotune=False, share_params=s.engine)
    # a layer the source lacks keeps its own filler-initialised storage
    txt = open(net_file).read().replace('"cvg/classifier"', '"cvg/other"')
    renamed = tmp_path / "renamed.prototxt"
    renamed.write_text(txt)
    spec, shapes = test_spec(str(renamed), mod)
    te = Engine(spec, shapes, None, device=0, autotune=False, share_params=s.engine)
    assert "cvg/other" not in te.shared_layers and "bbox/regressor" in te.shared_layers and te.param_count > 0
    lo, hi = te.param_flat.ptr, te.param_flat.ptr + te.param_flat.nbytes
    assert all(lo <= v.ptr < hi for v in te.params_dev["cvg/other"])
    want = fill_params(spec, seed=0)["cvg/other"]
    assert np.array_equal(te.read_param("cvg/other", 0), want[0]) and np.array_equal(te.read_param("cvg/other", 1), want[1])
    te.set_params("cvg/other", [w + 1 for w in want])      # its own storage: allowed
    te.close()
    s.close()


# ---- schedule and values ------------------------------------------------------------------------------------------------------------
def train_losses(lines):
    return [l.split("loss = ")[1] for l in lines if l.startswith("Iteration") and ", loss = " in l]


def passes_at(lines):
    return [int(l.split()[1].rstrip(",")) for l in lines if "Testing net (#0)" in l]


def test_schedule_values_and_undisturbed_training(gpu, tmp_path, layer_module):
    mod = layer_module
    job, net_file = write_job(tmp_path)
    lines = []
    s = Solver(job, device=0, log=lines.append, autotune=False)
    assert len(s.test_nets) == 1 and s.test_results == [None]
    assert s.test_nets[0].engine.shapes["data"] == (1, 3, 64, 96) and s.engine.shapes["data"] == (2, 3, 64, 64)
    s.step(3)      # tests at the top of iterations 0 and 2; the snapshot of iteration 2 lies between them
    assert passes_at(lines) == [0, 2]
    at2 = {k: v.copy() for k, v in s.test_results[0].items()}
    out_lines = [l for l in lines if "Test net output #" in l][-2:]
    losses_so_far = len(train_losses(lines))
    s.solve()
    assert passes_at(lines) == [0, 2, 4] and losses_so_far == 3 and len(train_losses(lines)) == 4
    # the pycaffe view reads the solver's weights in place
    view = s.test_nets[0]
    assert np.array_equal(bits(view.params["cvg/classifier"][1].data), bits(s.net.params["cvg/classifier"][1].data))
    assert set(view.forward()) == {"loss_bbox", "loss_coverage"} and view.blobs["coverage"].data.shape == (1, 2, 4, 6)
    s.close()

    # a standalone TEST engine on the iteration-2 snapshot and the same three batches (the second pass drew batches 3, 4, 5)
    spec, shapes = test_spec(net_file, mod)
    params = proto.read_caffemodel(str(tmp_path / "snap_iter_2.caffemodel"))
    alone = Engine(spec, shapes, params, device=0, autotune=False)
    cfg = mod.parse(TEST_CFG)
    outs = [forward_on(alone, mod.batch(cfg, k)) for k in (3, 4, 5)]
    alone.close()
    weights = {"loss_bbox": 2.0, "loss_coverage": 1.0}
    for j, name in enumerate(("loss_bbox", "loss_coverage")):
        want = E.test_mean([o[name] for o in outs])
        assert np.array_equal(bits(at2[name]), bits(want)), (name, at2[name], want)
        assert not np.array_equal(bits(want), bits(outs[0][name]))      # (the batches do differ)
        w = weights[name]
        assert out_lines[j] == "    Test net output #%d: %s = %g (* %g = %g loss)" % (j, name, want, w, w * want), out_lines[j]

    # the same job without a test net: bit-identical training
    plain_job, _ = write_job(tmp_path, test=False)
    plain_lines = []
    p = Solver(plain_job, device=0, log=plain_lines.append, autotune=False)
    assert p.test_nets == []
    p.solve()
    assert passes_at(plain_lines) == [] and train_losses(plain_lines) == train_losses(lines)
    a, b = proto.read_caffemodel(str(tmp_path / "snap_iter_4.caffemodel")), proto.read_caffemodel(str(tmp_path / "plain_iter_4.caffemodel"))
    for name in a:
        for x, y in zip(a[name], b[name]):
            assert np.array_equal(bits(x), bits(y)), name
    p.close()


def test_no_test_at_iteration_zero_without_test_initialization(gpu, tmp_path, layer_module):
    job, _ = write_job(tmp_path, extra="test_initialization: false\ntest_compute_loss: true\n")
    lines = []
    s = Solver(job, device=0, log=lines.append, autotune=False)
    s.step(2)
    assert passes_at(lines) == []
    s.step(1)
    assert passes_at(lines) == [2]
    loss_line = [l for l in lines if l.startswith("Test loss: ")]
    r = s.test_results[0]
    assert len(loss_line) == 1 and abs(float(loss_line[0].split(": ")[1]) - (2.0 * r["loss_bbox"] + r["loss_coverage"])) < 1e-4 * abs(
        2.0 * r["loss_bbox"] + r["loss_coverage"])
    s.close()


# ---- the bundled data layer in both phases -----------------------------------------------------------------------------------------
def test_bundled_data_layer_feeds_the_test_net_on_the_device(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("FCN_DATA_SEED", "3")
    sys.path.insert(0, PYCAFFE)
    net = tmp_path / "train_val.prototxt"
    # (the net's stride is 8 in both phases - label grids of another stride would not fit its heads - so the TEST copy differs in
    # image size and batch size)
    net.write_text(models.vgg16_bounding_box_train("data_argumentation_layer", "DataArgumentationLayer", "64,64,8,2,2,synthetic:2,detectnet",
                                                   num_classes=2, test_param_str="128,128,8,2,3,synthetic:2,detectnet"))
    solver = tmp_path / "solver.prototxt"
    solver.write_text('net: "%s"\nbase_lr: 1e-5\nsolver_type: ADAM\nmomentum: 0.9\nmomentum2: 0.999\nlr_policy: "fixed"\ndisplay: 1\nmax_iter: 2\n'
                      'test_iter: 2\ntest_interval: 2\nsnapshot_prefix: "%s"\n' % (net, tmp_path / "snap"))
    lines = []
    s = Solver(str(solver), device=0, log=lines.append, autotune=False)
    tn = s.test_nets[0]
    assert tn.engine.shapes["data"] == (3, 3, 128, 128) and s.engine.shapes["data"] == (2, 3, 64, 64)
    assert not tn.host_fed and tn.engine.device_fed == set(tn.engine.inputs)      # scenes rendered, label grids generated in HBM
    res = s.test_all()[0]
    assert tn.engine.score_forwards == 2
    assert set(res) == {"loss_bbox", "loss_coverage"} and all(np.isfinite(v).all() and v.shape == () for v in res.values())
    assert float(tn.blobs["coverage-label"].data.sum()) > 0      # the last batch had objects, labelled on the device
    s.step(2)
    assert passes_at(lines) == [0, 0] and all(np.isfinite(float(v)) for v in train_losses(lines))
    s.close()


# ---- Accuracy inside a net ------------------------------------------------------------------------------------------------------------
ACC_NET = """
name: "tiny_fcn"
input: "data" input_shape { dim: 2 dim: 3 dim: 16 dim: 20 }
input: "label" input_shape { dim: 2 dim: 1 dim: 16 dim: 20 }
layer { name: "conv1" type: "Convolution" bottom: "data" top: "conv1" param { lr_mult: 1 } param { lr_mult: 2 }
  convolution_param { num_output: 8 kernel_size: 3 pad: 1 weight_filler { type: "gaussian" std: 0.3 } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "relu1" type: "ReLU" bottom: "conv1" top: "conv1" }
layer { name: "score" type: "Convolution" bottom: "conv1" top: "score" param { lr_mult: 1 } param { lr_mult: 2 }
  convolution_param { num_output: 5 kernel_size: 1 weight_filler { type: "gaussian" std: 0.5 } bias_filler { type: "constant" value: 0 } } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "score" bottom: "label" top: "loss" loss_param { ignore_label: 255 normalize: true } }
%s
"""
ACC_LAYER = ('layer { name: "accuracy" type: "Accuracy" bottom: "score" bottom: "label" top: "accuracy" top: "per_class" '
             'accuracy_param { top_k: 1 ignore_label: 255 } }')


def acc_inputs():
    rng = np.random.default_rng(11)
    data = rng.standard_normal((2, 3, 16, 20)).astype(np.float32)
    label = rng.integers(0, 5, (2, 1, 16, 20)).astype(np.float32)
    label[rng.random(label.shape) < 0.15] = 255
    return data, label


def test_accuracy_layer_in_a_test_net_matches_the_reference_net(gpu):
    from oracle.net_ref import RefNet
    msg, plain = proto.parse_text(ACC_NET % ACC_LAYER), proto.parse_text(ACC_NET % "")
    spec = NetSpec(msg, "TEST")
    spec.infer()
    params = fill_params(spec, seed=5)
    eng = Engine(NetSpec(msg, "TEST"), params=params, device=0, autotune=False)
    assert eng.outputs == ["loss", "accuracy", "per_class"] and eng.shapes["per_class"] == (5,)
    data, label = acc_inputs()
    eng.host_array("data")[...] = data
    eng.host_array("label")[...] = label
    out = {k: v.copy() for k, v in eng.forward().items()}
    ref = RefNet(plain, "TEST", params)
    ref.blobs["data"], ref.blobs["label"] = data, label
    ref.forward()
    for score in (eng.read_blob("score"), ref.blobs["score"]):
        acc, per = E.accuracy(score, label, 1, 255)
        assert bits(out["accuracy"]) == bits(acc) and np.array_equal(bits(out["per_class"]), bits(per))
    assert 0.0 < float(out["accuracy"]) < 1.0
    eng.close()
    with pytest.raises(NotImplementedError, match="accuracy"):      # the half-float engine names the layer it cannot run
        only = "\n".join(l for l in (ACC_NET % ACC_LAYER).splitlines() if "SoftmaxWithLoss" not in l)      # (no half-float loss either)
        Engine(NetSpec(proto.parse_text(only), "TEST"), params=params, device=0, autotune=False, dtype="f16")


def test_accuracy_layer_leaves_a_training_step_unchanged(gpu):
    data, label = acc_inputs()
    got = []
    for extra in (ACC_LAYER, ""):
        msg = proto.parse_text(ACC_NET % extra)
        spec = NetSpec(msg, "TRAIN")
        spec.infer()
        te = TrainEngine(NetSpec(msg, "TRAIN"), {}, fill_params(spec, seed=5), device=0, solver=SolverParams(base_lr=0.01, momentum=0.9),
                         autotune=False)
        assert list(te.loss_blobs) == ["loss"]
        te.host_array("data")[...] = data
        te.host_array("label")[...] = label
        losses = [te.step()["total_loss"] for _ in range(2)]
        got.append((losses, te.download_grads(), te.download_params()))
        if extra:
            acc, per = E.accuracy(te.read_blob("score"), label, 1, 255)
            assert bits(te.read_blob("accuracy")) == bits(acc) and np.array_equal(bits(te.read_blob("per_class")), bits(per))
        te.close()
    assert got[0][0] == got[1][0]
    for which in (1, 2):
        for name in got[0][which]:
            for x, y in zip(got[0][which][name], got[1][which][name]):
                assert np.array_equal(bits(x), bits(y)), name


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------
def test_caffe_test_tool_scores_a_snapshot(gpu, tmp_path, layer_module):
    job, net_file = write_job(tmp_path, extra="test_initialization: false\n", max_iter=2)
    s = Solver(job, device=0, log=None, autotune=False)
    s.solve()      # (writes snap_iter_2 and runs the pass of iteration 2: the layer instance of the solver has moved on)
    s.close()
    weights = str(tmp_path / "snap_iter_2.caffemodel")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), PYCAFFE, os.environ.get("PYTHONPATH", "")]), FCN_AUTOTUNE="0")
    r = subprocess.run([sys.executable, CAFFE, "test", "--model=%s" % net_file, "--weights=%s" % weights, "--iterations=4", "--gpu=0"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    log = [l.split(" ", 2)[2] for l in r.stderr.splitlines() if l.startswith("I") and l.count(" ") >= 2]
    for k in range(4):
        assert [l.split(", ")[1].split(" = ")[0] for l in log if l.startswith("Batch %d, " % k)] == ["loss_bbox", "loss_coverage"]
    assert not any(l.startswith("Batch 4, ") for l in log) and any(l.startswith("Loss: ") for l in log)
    # Solver.test(0) on the same weights and the same batches (a fresh layer instance starts at batch 0 again)
    job4 = tmp_path / "solver4.prototxt"
    job4.write_text(open(job).read().replace("test_iter: 3", "test_iter: 4"))
    s = Solver(str(job4), device=0, log=None, autotune=False)
    s.net.copy_from(weights)
    means = s.test(0)
    s.close()
    tail = log[log.index([l for l in log if l.startswith("Loss: ")][0]) + 1:]
    assert tail[:2] == ["loss_bbox = %g (* 2 = %g loss)" % (means["loss_bbox"], 2.0 * means["loss_bbox"]),
                        "loss_coverage = %g (* 1 = %g loss)" % (means["loss_coverage"], means["loss_coverage"])], tail


# ---- pycaffe: Net.share_with -------------------------------------------------------------------------------------------------------------
def test_pycaffe_share_with_reads_the_other_nets_storage(gpu, tmp_path):
    sys.path.insert(0, PYCAFFE)
    import caffe
    path = tmp_path / "tiny.prototxt"
    path.write_text(ACC_NET % ACC_LAYER)
    data, label = acc_inputs()
    a, b = caffe.Net(str(path), caffe.TEST), caffe.Net(str(path), caffe.TEST)
    a.params["score"][1].data[...] = np.arange(5, dtype=np.float32)
    out_a = {k: v.copy() for k, v in a.forward(data=data, label=label).items()}
    out_b = {k: v.copy() for k, v in b.forward(data=data, label=label).items()}
    assert not np.array_equal(bits(out_a["loss"]), bits(out_b["loss"]))
    b.share_with(a)
    assert b._engine.shared_layers == {"conv1", "score"}
    out_b = {k: v.copy() for k, v in b.forward(data=data, label=label).items()}
    for k in out_a:
        assert np.array_equal(bits(out_a[k]), bits(out_b[k])), k
    a.params["score"][1].data[...] = 0      # an edit through the owner, uploaded at ITS next forward, reaches both
    out_a2 = {k: v.copy() for k, v in a.forward(data=data, label=label).items()}
    out_b2 = {k: v.copy() for k, v in b.forward(data=data, label=label).items()}
    assert not np.array_equal(bits(out_a2["loss"]), bits(out_a["loss"]))
    for k in out_a2:
        assert np.array_equal(bits(out_a2[k]), bits(out_b2[k])), k
    other = tmp_path / "other.prototxt"
    other.write_text((ACC_NET % ACC_LAYER).replace("num_output: 5", "num_output: 6"))
    c = caffe.Net(str(other), caffe.TEST)
    with pytest.raises(ValueError, match="score"):
        c.share_with(a)
    assert c.forward(data=data, label=label)["loss"].shape == ()      # still usable with its own weights
