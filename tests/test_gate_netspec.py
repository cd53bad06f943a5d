"""The scale_gate opt-in, the two layer forms it admits and the SE-ResNet writer - without a GPU.

A Scale with two bottoms (x, gate) over axis 0 and the SENet release's Axpy (gate, x, residual): shapes, the Axpy lowering (names,
blobs, no parameters), every refusal by layer name, a bare NetSpec as before, the public entry points passing the keyword, and
models.se_resnet in three phases and both forms."""
import sys

import pytest

from conftest import PYCAFFE
from fcn_object_detector_amd import caffe_tool, engine, models, proto, solver, train
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd.netspec import NetSpec, fill_params, is_scale_gate, scale_gate_form

HEAD = """
input: "data" input_shape { dim: 3 dim: 12 dim: 5 dim: 7 }
input: "g" input_shape { dim: 3 dim: 12 }
input: "g4" input_shape { dim: 3 dim: 12 dim: 1 dim: 1 }
input: "res" input_shape { dim: 3 dim: 12 dim: 5 dim: 7 }
input: "flat" input_shape { dim: 3 dim: 12 }
input: "one" input_shape { dim: 3 dim: 12 dim: 1 dim: 1 }
input: "gc" input_shape { dim: 12 }
input: "gn" input_shape { dim: 3 }
input: "gnc5" input_shape { dim: 3 dim: 12 dim: 5 }
"""


def spec_of(layers, phase="TEST", **kw):
    s = NetSpec(proto.parse_text(HEAD + layers), phase, **dict(dict(scale_gate=True), **kw))
    s.infer()
    return s


def scale(name, x, g, top=None, extra="axis: 0"):
    return 'layer { name: "%s" type: "Scale" bottom: "%s" bottom: "%s" top: "%s" scale_param { %s } }\n' % (name, x, g, top or name, extra)


def test_the_keyword():
    msg = proto.parse_text(HEAD)
    assert NetSpec(msg).scale_gate is False and NetSpec(msg, "TEST", True, True, True, True).scale_gate is False
    assert NetSpec(msg, "TEST", False, False, False, False, True).scale_gate is True and NetSpec(msg, scale_gate=1).scale_gate is True


def test_from_file_takes_it_by_keyword_only(tmp_path):
    p = tmp_path / "net.prototxt"
    p.write_text(HEAD + scale("sc", "data", "g"))
    assert NetSpec.from_file(str(p)).scale_gate is False
    s = NetSpec.from_file(str(p), "TRAIN", scale_gate=True)
    assert s.scale_gate is True and s.ip_gemm is False and s.phase == "TRAIN" and s.infer()["sc"] == (3, 12, 5, 7)
    with pytest.raises(TypeError):
        NetSpec.from_file(str(p), "TEST", False, True)


def test_the_gated_scale_has_the_shape_of_x_and_no_parameters():
    s = spec_of(scale("sc", "data", "g") + scale("sc2", "flat", "g") + scale("sc4", "one", "g4") + scale("scn", "data", "g", extra="axis: -4"))
    assert s.blob_shapes["sc"] == s.blob_shapes["scn"] == (3, 12, 5, 7) and s.blob_shapes["sc2"] == (3, 12) and s.blob_shapes["sc4"] == (3, 12, 1, 1)
    assert s.param_shapes == {} and s.param_layers() == [] and fill_params(s) == {}
    assert all(is_scale_gate(l) for l in s.layers)
    assert scale_gate_form(s.layers[0], [(3, 12, 5, 7), (3, 12)], "TEST") == (3, 35, 12)
    assert scale_gate_form(s.layers[1], [(3, 12), (3, 12)], "TRAIN") == (3, 1, 12)
    # in place on x is Caffe's too - in a TEST net
    assert spec_of(scale("sc", "data", "g", top="data")).blob_shapes["data"] == (3, 12, 5, 7)


def test_a_learned_scale_is_what_it_was():
    text = 'layer { name: "s" type: "Scale" bottom: "data" top: "s" scale_param { bias_term: true } }\n'
    assert spec_of(text).param_shapes == spec_of(text, scale_gate=False).param_shapes == {"s": [(12,), (12,)]}
    assert not is_scale_gate(spec_of(text).layers[0])


REFUSED = [
    (scale("sb", "data", "g", extra="axis: 0 bias_term: true"), NotImplementedError, "sb.*bias_term"),
    (scale("s1", "data", "gc", extra="axis: 1"), NotImplementedError, "s1.*axis 1"),
    (scale("sd", "data", "gc", extra=""), NotImplementedError, "sd.*axis 1"),                     # (Caffe's default axis is 1)
    (scale("sn", "data", "gn"), NotImplementedError, "sn.*1-d multiplier"),
    (scale("sf", "data", "res"), NotImplementedError, "sf.*4-d multiplier"),
    (scale("s3", "data", "gnc5"), NotImplementedError, "s3.*3-d multiplier"),
    (scale("sm", "data", "g4"), ValueError, "sm.*does not match"),                                # (N, C, 1, 1) where H x W is 5 x 7: Caffe's rule
    (scale("sx", "data", "gc"), ValueError, "sx.*does not match"),
    (scale("sa", "data", "g", extra="axis: 7"), ValueError, "sa.*axis 7"),
    (scale("sg", "data", "g", top="g"), ValueError, "sg.*over the multiplier"),
    ('layer { name: "a2" type: "Axpy" bottom: "g" bottom: "data" top: "a2" }\n', ValueError, "a2.*three bottoms"),
]


@pytest.mark.parametrize("layer,kind,match", REFUSED)
def test_refusals_by_layer_name(layer, kind, match):
    with pytest.raises(kind, match=match):
        spec_of(layer)


def test_in_place_on_x_is_refused_in_a_train_net():
    with pytest.raises(NotImplementedError, match="Scale with two bottoms in place on data in a TRAIN net"):
        spec_of(scale("sc", "data", "g", top="data"), "TRAIN")
    assert spec_of(scale("sc", "data", "g"), "TRAIN").blob_shapes["sc"] == (3, 12, 5, 7)


def test_a_bare_netspec_refuses_as_before_and_says_how_to_opt_in():
    with pytest.raises(NotImplementedError, match=r"layer sc: Scale with two bottoms \(the multiplier as a blob of the net\).*"
                                                  r"NetSpec built with scale_gate=True \(caffe.Net, the solvers and the caffe tool pass it\)"):
        spec_of(scale("sc", "data", "g"), scale_gate=False)
    with pytest.raises(NotImplementedError, match=r"layer type 'Axpy' \(layer ax\)"):
        spec_of('layer { name: "ax" type: "Axpy" bottom: "g4" bottom: "data" bottom: "res" top: "ax" }\n', scale_gate=False)


@pytest.mark.parametrize("gate", ["g4", "g"])
def test_the_axpy_lowering(gate):
    s = spec_of('layer { name: "ax" type: "Axpy" bottom: "%s" bottom: "data" bottom: "res" top: "out" }\n'
                'layer { name: "ax/relu" type: "ReLU" bottom: "out" top: "out" }\n' % gate)
    assert [(l.name, l.type, l.bottoms, l.tops) for l in s.layers] == [
        ("ax/scale", "Scale", ["data", gate], ["out/scale"]), ("ax", "Eltwise", ["out/scale", "res"], ["out"]), ("ax/relu", "ReLU", ["out"], ["out"])]
    assert [l.axpy for l in s.layers] == ["ax", "ax", None] and int(s.layers[0].sub("scale_param").get("axis")) == 0
    assert s.blob_shapes["out/scale"] == s.blob_shapes["out"] == (3, 12, 5, 7) and s.param_shapes == {}
    assert not any(l.type == "Axpy" for l in s.layers)


def test_an_axpy_of_another_phase_is_left_out():
    s = spec_of('layer { name: "ax" type: "Axpy" bottom: "g" bottom: "data" bottom: "res" top: "out" include { phase: TRAIN } }\n')
    assert s.layers == []


# ---------------------------------------------------------------------------------------------------------------- public entry points
NET = HEAD.replace('input: "g4"', 'input: "unused4"') + scale("sc", "data", "g")


class Stop(Exception):
    pass


@pytest.fixture
def recorded(monkeypatch, tmp_path):
    """(specs, net file, solver file): every NetSpec built from here on is appended to specs; engines stop in their constructor"""
    specs = []
    init = NetSpec.__init__

    def recording(self, *a, **kw):
        init(self, *a, **kw)
        specs.append(self)

    def stop(self, spec, *a, **kw):
        assert spec in specs
        raise Stop()
    monkeypatch.setattr(NetSpec, "__init__", recording)
    monkeypatch.setattr(engine.Engine, "__init__", stop)
    monkeypatch.setattr(train.TrainEngine, "__init__", stop)
    monkeypatch.setattr(L, "call", lambda name, *a: None)
    net = tmp_path / "net.prototxt"
    net.write_text(NET)
    sol = tmp_path / "solver.prototxt"
    sol.write_text('net: "%s"\nbase_lr: 0.01\nlr_policy: "fixed"\nmax_iter: 1\n' % net)
    return specs, str(net), str(sol)


def opted_in(specs, phase):
    return len(specs) >= 1 and all(s.scale_gate and s.phase == phase for s in specs)


def test_the_public_entry_points_pass_it(recorded, tmp_path):
    specs, net, sol = recorded
    sys.path.insert(0, PYCAFFE)
    try:
        import caffe
        for phase, name in ((caffe.TEST, "TEST"), (caffe.TRAIN, "TRAIN")):
            del specs[:]
            with pytest.raises(Stop):
                caffe.Net(net, phase)
            assert opted_in(specs, name), name
    finally:
        sys.path.remove(PYCAFFE)
    weights = tmp_path / "w.caffemodel"
    weights.write_bytes(b"")
    for make, phase in ((lambda: solver.Solver(sol, log=None), "TRAIN"), (lambda: solver.get_solver(sol, log=None), "TRAIN"),
                        (lambda: solver.TestNet(net), "TEST"), (lambda: caffe_tool.main(["time", "--model", net]), "TEST"),
                        (lambda: caffe_tool.main(["test", "--model", net, "--weights", str(weights)]), "TEST"),
                        (lambda: caffe_tool.main(["train", "--solver", sol]), "TRAIN")):
        del specs[:]
        with pytest.raises(Stop):
            make()
        assert opted_in(specs, phase), phase


# ---------------------------------------------------------------------------------------------------------------- the writer
KW = dict(depth=50, width_div=8, size=64, batch=2, num_classes=10, reduction=4)


@pytest.mark.parametrize("phase", ["DEPLOY", "TEST", "TRAIN"])
def test_se_resnet_in_three_phases_and_both_forms(phase):
    specs = {}
    for form in ("scale", "axpy"):
        txt = models.se_resnet(phase, form=form, **KW)
        assert ('type: "Axpy"' in txt) == (form == "axpy") and ('type: "InnerProduct"' in txt)
        assert txt.count('type: "Sigmoid"') == 16 and txt.count("global_pooling: true") == 17
        specs[form] = s = NetSpec(proto.parse_text(txt), "TRAIN" if phase == "TRAIN" else "TEST", scale_gate=True)
        shapes = s.infer()
        assert shapes["conv2_1"] == (2, 32, 16, 16) and shapes["conv5_3"] == (2, 256, 2, 2) and shapes["conv2_1/scale"] == shapes["conv2_1"]
        assert shapes["conv2_1_1x1_down"][:2] == (2, 8) and shapes["conv5_3_1x1_down"][:2] == (2, 64) and shapes["conv5_3_prob"][:2] == (2, 256)
        assert len([l for l in s.layers if is_scale_gate(l)]) == 16 and not [l for l in s.layers if l.type == "Axpy"]
        assert s.output_blobs() == (["prob"] if phase == "DEPLOY" else ["accuracy", "loss"] if phase == "TEST" else ["loss"])
        with pytest.raises(NotImplementedError, match="conv2_1" if form == "axpy" else "conv2_1/scale: Scale with two bottoms"):
            NetSpec(proto.parse_text(txt), "TEST").infer()
    a, b = specs["scale"], specs["axpy"]
    assert [(l.name, l.bottoms, l.tops) for l in a.layers] == [(l.name, l.bottoms, l.tops) for l in b.layers]
    assert list(a.param_shapes) == list(b.param_shapes)
    for name in a.param_shapes:      # the same parameter shapes up to the trailing 1, 1 of the squeeze and excite layers
        strip = lambda shp: tuple(shp[:2]) if len(shp) == 4 and tuple(shp[2:]) == (1, 1) and name.endswith(("_1x1_down", "_1x1_up")) else tuple(shp)
        assert [strip(x) for x in a.param_shapes[name]] == [strip(x) for x in b.param_shapes[name]], name
    assert a.param_shapes["conv2_1_1x1_down"] == [(8, 32), (8,)] and b.param_shapes["conv2_1_1x1_down"] == [(8, 32, 1, 1), (8,)]


def test_se_resnet_depths_and_arguments():
    for depth, fn, blocks in ((50, models.se_resnet50, 16), (101, models.se_resnet101, 33), (152, models.se_resnet152, 50)):
        txt = fn("DEPLOY", width_div=8, size=64)
        assert txt == models.se_resnet("DEPLOY", depth=depth, width_div=8, size=64) and txt.count('type: "Sigmoid"') == blocks
    s = NetSpec(proto.parse_text(models.se_resnet50()), "TEST", scale_gate=True)
    shapes = s.infer()
    assert shapes["conv2_1_1x1_down"] == (1, 16) and shapes["conv5_3_1x1_down"] == (1, 128) and shapes["prob"] == (1, 1000)
    assert "_filler" not in models.se_resnet(fillers=False, width_div=8, size=64)
    for bad in (dict(depth=18), dict(form="bias"), dict(reduction=0), dict(phase="VAL")):
        with pytest.raises(ValueError):
            models.se_resnet(**dict(dict(width_div=8, size=64), **bad))
