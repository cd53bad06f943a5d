"""ArgMax as the forward planner lays it out - without a GPU, on the stub engine of tests/plan_stub.py (DeviceBuffer replaced by
a counter of addresses, the library by one whose every entry point returns 0 and records its name).

Checked: the launch list of the three fused forms and the entry point each launch calls; the launch list for each reason not to
fuse (a second reader, a net output, top_k 2 behind an Interp, fuse=False); the blobs a fused launch skips and the launches that
fill them on demand; the float32 top in the half-float plan; that a TRAIN net with an ArgMax beside its loss plans both passes."""
import pytest

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd.netspec import NetSpec
from plan_stub import engine_factory

FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'
HEAD = """
input: "data" input_shape { dim: 2 dim: 3 dim: 5 dim: 6 }
layer { name: "score" type: "Convolution" bottom: "data" top: "score" convolution_param { num_output: 7 kernel_size: 3 pad: 1 %s } }
""" % FILL
INTERP = 'layer { name: "up" type: "Interp" bottom: "score" top: "up" interp_param { zoom_factor: 3 } }\n'
SOFTMAX = 'layer { name: "prob" type: "Softmax" bottom: "%s" top: "prob" }\n'
ARGMAX = 'layer { name: "am" type: "ArgMax" bottom: "%s" top: "am" argmax_param { axis: 1 %s } }\n'
RELU = 'layer { name: "more" type: "ReLU" bottom: "%s" top: "more" }\n'


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, backward=False)


def launches(e):
    return [(op.kind, op.name) for t in e.tasks if isinstance(t, E.OpTask) for op in t.ops]


def called(e, op):
    del e.fake.calls[:]
    op.run(None)
    return e.fake.names()


def argmax_op(e):
    ops = [op for t in e.tasks if isinstance(t, E.OpTask) for op in t.ops if op.kind == "argmax"]
    assert len(ops) == 1
    return ops[0]


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_the_three_fused_forms_are_one_launch(stub, f16):
    sfx = "_f16" if f16 else "_f32"
    e = stub(HEAD + INTERP + ARGMAX % ("up", ""), f16=f16)
    assert launches(e) == [("argmax", "up+am")] and sorted(e._lazy_blob_ops) == ["up"]
    assert called(e, argmax_op(e)) == ["fcn_interp_argmax_fwd" + sfx]
    assert [op.kind for op in e._lazy_blob_ops["up"]] == ["interp"]
    e = stub(HEAD + SOFTMAX % "score" + ARGMAX % ("prob", "out_max_val: true top_k: 2"), f16=f16)
    assert launches(e) == [("argmax", "prob+am")] and sorted(e._lazy_blob_ops) == ["prob"]
    assert called(e, argmax_op(e)) == ["fcn_argmax_fwd" + sfx]
    assert [op.kind for op in e._lazy_blob_ops["prob"]] == ["softmax"]
    e = stub(HEAD + INTERP + SOFTMAX % "up" + ARGMAX % ("prob", ""), f16=f16)
    assert launches(e) == [("argmax", "up+prob+am")] and sorted(e._lazy_blob_ops) == ["prob", "up"]
    assert called(e, argmax_op(e)) == ["fcn_interp_argmax_fwd" + sfx]
    assert [op.kind for op in e._lazy_blob_ops["up"]] == ["interp"] and [op.kind for op in e._lazy_blob_ops["prob"]] == ["interp", "softmax"]
    # bytes: the small map in, one float per output pixel out; no FLOPs are booked
    op, esz = argmax_op(e), 2 if f16 else 4
    assert op.flops == 0.0 and op.bytes == esz * 2 * 5 * 6 * 7 + 4.0 * 2 * 13 * 16


def test_the_flags_of_each_form(stub, monkeypatch):
    seen = []
    fake = stub(HEAD + ARGMAX % ("score", "")).fake      # (one library object serves every engine of a test: record before planning)
    monkeypatch.setattr(fake, "fcn_argmax_fwd_f32", lambda *a: seen.append(a) or 0, raising=False)
    for tail, want in ((ARGMAX % ("score", ""), 0), (ARGMAX % ("score", "out_max_val: true"), L.ARGMAX_VALUES),
                       (SOFTMAX % "score" + ARGMAX % ("prob", ""), L.ARGMAX_SOFTMAX),
                       (SOFTMAX % "score" + ARGMAX % ("prob", "out_max_val: true top_k: 3"), L.ARGMAX_SOFTMAX | L.ARGMAX_VALUES)):
        e = stub(HEAD + tail)
        argmax_op(e).run(None)
        x, y = e.blobs["score"], e.blobs["am"]
        k = 3 if "top_k: 3" in tail else 1
        assert seen[-1] == (x.buf.ptr, y.buf.ptr, 2 * 5 * 6, 7, x.cstride, x.coffset, k, y.cstride, y.coffset, want, None)
    # the classifier's legacy form: indices, then values, in one row per image
    e = stub('input: "fc" input_shape { dim: 3 dim: 40 }\n' + SOFTMAX % "fc" +
             'layer { name: "am" type: "ArgMax" bottom: "prob" top: "am" argmax_param { top_k: 5 out_max_val: true } }')
    argmax_op(e).run(None)
    y = e.blobs["am"]
    assert y.shape == (3, 2, 5) and y.nchw == (3, 10, 1, 1) and y.cstride == 12
    assert seen[-1][2:] == (3, 40, 40, 0, 5, 12, 0, L.ARGMAX_SOFTMAX | L.ARGMAX_PAIRS, None)


def test_each_reason_not_to_fuse(stub, monkeypatch):
    # a second reader of the blob in front
    e = stub(HEAD + INTERP + ARGMAX % ("up", "") + RELU % "up")
    assert launches(e) == [("interp", "up"), ("argmax", "am"), ("relu", "more")] and not e._lazy_blob_ops
    e = stub(HEAD + INTERP + SOFTMAX % "up" + ARGMAX % ("prob", "") + RELU % "prob")
    assert launches(e) == [("interp", "up"), ("softmax", "prob"), ("argmax", "am"), ("relu", "more")]
    e = stub(HEAD + INTERP + SOFTMAX % "up" + RELU % "up" + ARGMAX % ("prob", ""))      # the Interp stays out, the Softmax rides
    assert launches(e) == [("interp", "up"), ("argmax", "prob+am"), ("relu", "more")] and sorted(e._lazy_blob_ops) == ["prob"]
    # top_k 2 behind an Interp: the fused pass keeps one pair per pixel
    e = stub(HEAD + INTERP + ARGMAX % ("up", "top_k: 2"))
    assert launches(e) == [("interp", "up"), ("argmax", "am")]
    e = stub(HEAD + INTERP + SOFTMAX % "up" + ARGMAX % ("prob", "top_k: 2"))
    assert launches(e) == [("interp", "up"), ("argmax", "prob+am")]
    # a net output: a caller that asks for the probabilities too gets two launches
    keep = NetSpec.output_blobs
    monkeypatch.setattr(NetSpec, "output_blobs", lambda self: ["prob"] + keep(self))
    e = stub(HEAD + SOFTMAX % "score" + ARGMAX % ("prob", ""))
    assert e.outputs == ["prob", "am"] and launches(e) == [("softmax", "prob"), ("argmax", "am")] and not e._lazy_blob_ops
    monkeypatch.setattr(NetSpec, "output_blobs", keep)
    # fuse=False
    e = stub(HEAD + INTERP + SOFTMAX % "up" + ARGMAX % ("prob", ""))
    e.fuse, e._lazy_blob_ops = False, {}
    e.tasks = e._collect_tasks()
    assert launches(e) == [("interp", "up"), ("softmax", "prob"), ("argmax", "am")] and not e._lazy_blob_ops


def test_the_top_is_float32_in_the_half_float_plan(stub):
    e = stub(HEAD + INTERP + ARGMAX % ("up", ""), f16=True)
    assert (e.blobs["score"].esize, e.blobs["up"].esize, e.blobs["am"].esize) == (2, 2, 4)
    e = stub(HEAD + ARGMAX % ("score", "top_k: 3 out_max_val: true"), f16=True)
    assert e.blobs["am"].esize == 4 and called(e, argmax_op(e)) == ["fcn_argmax_fwd_f16"]
    # a half-float reader of the top is refused by layer name
    with pytest.raises(NotImplementedError) as err:
        stub(HEAD + ARGMAX % ("score", "") + RELU % "am", f16=True)
    assert "more" in str(err.value) and "ArgMax am" in str(err.value)
    e = stub(HEAD + ARGMAX % ("score", "") + RELU % "am")      # the float32 engine reads it like any blob
    assert launches(e) == [("argmax", "am"), ("relu", "more")]


def test_a_train_net_with_an_argmax_beside_the_loss_plans_both_passes(stub):
    text = ('input: "label" input_shape { dim: 2 dim: 1 dim: 5 dim: 6 }\n' + HEAD + ARGMAX % ("score", "") +
            'layer { name: "loss" type: "SoftmaxWithLoss" bottom: "score" bottom: "label" top: "loss" }\n')
    e = stub(text, phase="TRAIN")
    assert ("argmax", "am") in launches(e) and e.outputs == ["am", "loss"]
    plan = BW.BackwardPlanner(e)
    assert "ArgMax" not in plan.emitters and "ArgMax" not in plan.one_bottom      # no emitter: no gradient arrives at the layer
    am = {l.name: l for l in e.spec.layers}["am"]
    plan._one_bottom(am)
    assert plan.ops == []
    # a gradient that does arrive is refused by layer name, as Caffe refuses it
    plan.mark(e.grad_blobs["am"])
    with pytest.raises(NotImplementedError, match=r"backward of layer type ArgMax \(am\)"):
        plan._one_bottom(am)
