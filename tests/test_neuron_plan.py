"""ELU, ReLU6, Clip, AbsVal, BNLL and Swish (csrc/neuron.hip) as the forward and backward planners lay them out - without a GPU.

The stub engine of tests/plan_stub.py, on a bare NetSpec and on NetSpec.public's alike (the layers need no keyword).  Checked: one launch
per layer and its operands in both element types; a convolution's or a BatchNorm chain's fusion ends in front of a ReLU6; the kept copy
exists exactly where a gradient comes to an in-place Swish; windows and the refusals by layer name; the backward order, the blob each
gradient launch reads and its accumulate flag; that models.resnet and models.mtcnn - nets without one of these layers - plan as the parent
commit planned them (by the SHA-256 of their launch lists and storage plans, recorded there); and that models.efficientnet_b0 and
models.mobilenet_v2(relu6=True) plan completely, in float32 TRAIN and in halves."""
import hashlib

import pytest

from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import models
from plan_stub import engine_factory


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, public=True)


@pytest.fixture
def bare(monkeypatch):
    return engine_factory(monkeypatch)


def fwd_ops(e, kinds=("neuron",)):
    return [op for t in e.tasks if isinstance(t, E.OpTask) for op in t.ops if op.kind in kinds]


def run(e, ops):
    del e.fake.calls[:]
    for op in ops:
        op.run(None)
    return list(e.fake.calls)


DATA = 'layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 2 dim: 8 dim: 5 dim: 7 } } }\n'
CONV = 'layer { name: "x" type: "Convolution" bottom: "data" top: "x" convolution_param { num_output: 16 kernel_size: 3 pad: 1 } }\n'
FROZEN = CONV.replace('top: "x" ', 'top: "x" param { lr_mult: 0 } param { lr_mult: 0 } ')
OUT = 'layer { name: "out" type: "Convolution" bottom: "%s" top: "out" convolution_param { num_output: 8 kernel_size: 1 } }\n'
LOSS = ('layer { name: "target" type: "Input" top: "target" input_param { shape { dim: 2 dim: 8 dim: 5 dim: 7 } } }\n'
        'layer { name: "loss" type: "EuclideanLoss" bottom: "out" bottom: "target" top: "loss" }\n')
SIX = (DATA + CONV + 'layer { name: "e" type: "ELU" bottom: "x" top: "x" elu_param { alpha: 0.5 } }\n'
       'layer { name: "a" type: "AbsVal" bottom: "x" top: "a" }\n'
       'layer { name: "r" type: "ReLU6" bottom: "a" top: "a" }\n'
       'layer { name: "c" type: "Clip" bottom: "a" top: "c" clip_param { min: -1 max: 2 } }\n'
       'layer { name: "b" type: "BNLL" bottom: "c" top: "c" }\n'
       'layer { name: "s" type: "Swish" bottom: "c" top: "s" swish_param { beta: 1.5 } }\n' + OUT % "s")
MODES = [("e", L.NEURON_ELU, 0.5, 0.0), ("a", L.NEURON_ABSVAL, 0.0, 0.0), ("r", L.NEURON_CLIP, 0.0, 6.0), ("c", L.NEURON_CLIP, -1.0, 2.0),
         ("b", L.NEURON_BNLL, 0.0, 0.0), ("s", L.NEURON_SWISH, 1.5, 0.0)]


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("public", [False, True])
def test_one_launch_per_layer_in_both_element_types(stub, bare, f16, public):
    e = (stub if public else bare)(SIX, f16=f16)
    ops = fwd_ops(e)
    assert [op.name for op in ops] == ["e", "a", "r", "c", "b", "s"]
    B = e.blobs
    assert all(B[n].esize == (2 if f16 else 4) for n in ("x", "a", "c", "s")) and B["out"].esize == 4      # halves in, halves out; the output float32
    io = {"e": ("x", "x"), "a": ("x", "a"), "r": ("a", "a"), "c": ("a", "c"), "b": ("c", "c"), "s": ("c", "s")}
    calls = run(e, ops)
    pix, c = 2 * 5 * 7, 16
    for (fn, args), (name, mode, a, b) in zip(calls, MODES):
        x, y = B[io[name][0]], B[io[name][1]]
        if f16:
            assert (fn, args) == ("fcn_neuron_fwd_f16", (x.buf.ptr, y.buf.ptr, pix, c, x.cstride, x.coffset, y.cstride, y.coffset, mode, a, b, None)), name
        else:
            assert (fn, args) == ("fcn_neuron_fwd_f32", (x.buf.ptr, y.buf.ptr, None, pix, c, x.cstride, 0, y.cstride, 0, 16, mode, a, b, None)), name
    assert not e.aux_dev and not any(l.name in e.params_dev for l in e.spec.layers if l.name in io)      # a TEST engine keeps nothing; no blobs


def test_a_float32_net_output_of_one_of_them_stays_refused_in_halves(stub):
    for t, body in (("ELU", ""), ("ReLU6", ""), ("Clip", "clip_param { min: 0 max: 1 }"), ("AbsVal", ""), ("BNLL", ""), ("Swish", "")):
        layer = 'layer { name: "p" type: "%s" bottom: "x" top: "y" %s }' % (t, body)
        with pytest.raises(NotImplementedError, match="f16 engine: float32 blob y is produced by"):
            stub(DATA + CONV + layer, f16=True)
        assert [op.name for op in fwd_ops(stub(DATA + CONV + layer))] == ["p"]      # (float32: nothing to refuse)


def test_a_fusion_ends_in_front_of_a_relu6(stub):
    """As in front of a ReLU with a slope or a PReLU: the convolution epilogue and the BatchNorm chain recognise only a plain ReLU."""
    six = 'layer { name: "p" type: "ReLU6" bottom: "x" top: "x" }\n'
    e = stub(DATA + CONV + six + OUT % "x")
    assert e._conv_layer_meta["x"]["relu"] is False and not (e._conv_flags["x"] & L.CONV_RELU) and [op.name for op in fwd_ops(e)] == ["p"]
    relu = stub(DATA + CONV + 'layer { name: "p" type: "ReLU" bottom: "x" top: "x" }\n' + OUT % "x")
    assert relu._conv_layer_meta["x"]["relu"] and relu._conv_flags["x"] & L.CONV_RELU and not fwd_ops(relu, ("neuron", "relu"))
    chain = (DATA + CONV + 'layer { name: "bn" type: "BatchNorm" bottom: "x" top: "x" }\n'
             'layer { name: "sc" type: "Scale" bottom: "x" top: "x" scale_param { bias_term: true } }\n' + six + OUT % "x")
    for f16 in (False, True):
        e = stub(chain, f16=f16)
        ch = e._bn_chains["bn"]
        assert ch.scale is not None and ch.relu is None
        assert [(op.kind, op.name) for op in fwd_ops(e, ("bn_apply", "neuron", "relu"))] == [("bn_apply", "bn+sc"), ("neuron", "p")]
        (_, a), = run(e, fwd_ops(e, ("bn_apply",)))
        assert a[-2] == 0      # (the apply launch's relu flag)
    e = stub(DATA + 'layer { name: "ip" type: "InnerProduct" bottom: "data" top: "ip" inner_product_param { num_output: 12 } }\n'
             'layer { name: "p" type: "Swish" bottom: "ip" top: "ip" }\n')
    assert not e._conv_layer_meta["ip"]["relu"] and [op.name for op in fwd_ops(e)] == ["p"]
    (_, a), = run(e, fwd_ops(e))
    assert a[3:5] == (2, 12)      # a 2-d blob: N pixels of C channels


SW = 'layer { name: "p" type: "Swish" bottom: "x" top: "%s" }'
KEEP_CASES = [
    # (name, the layer, layers in front, phase, kept?)
    ("Swish in place, TRAIN, a gradient comes", SW % "x", CONV, "TRAIN", True),
    ("Swish in place, TRAIN, nothing in front learns", SW % "x", FROZEN, "TRAIN", False),
    ("Swish with a top of its own, TRAIN", SW % "y", CONV, "TRAIN", False),
    ("Swish in place, TEST", SW % "x", CONV, "TEST", False),
    ("ELU in place, TRAIN", 'layer { name: "p" type: "ELU" bottom: "x" top: "x" }', CONV, "TRAIN", False),
    ("ReLU6 in place, TRAIN", 'layer { name: "p" type: "ReLU6" bottom: "x" top: "x" }', CONV, "TRAIN", False),
    ("Clip in place, TRAIN", 'layer { name: "p" type: "Clip" bottom: "x" top: "x" clip_param { min: -1 max: 1 } }', CONV, "TRAIN", False),
    ("BNLL in place, TRAIN", 'layer { name: "p" type: "BNLL" bottom: "x" top: "x" }', CONV, "TRAIN", False),
    ("AbsVal, TRAIN", 'layer { name: "p" type: "AbsVal" bottom: "x" top: "y" }', CONV, "TRAIN", False),
]


@pytest.mark.parametrize("name,layer,front,phase,kept", KEEP_CASES, ids=[c[0] for c in KEEP_CASES])
def test_the_kept_copy_is_there_exactly_when_needed(stub, name, layer, front, phase, kept):
    top = "y" if 'top: "y"' in layer else "x"
    e = stub(DATA + front + layer + "\n" + OUT % top + LOSS, phase)
    assert ("p" in e.aux_dev) == kept
    (fn, a), = run(e, fwd_ops(e))
    x, y = e.blobs["x"], e.blobs[top]
    assert fn == "fcn_neuron_fwd_f32" and a[2] == (e.aux_dev["p"].ptr if kept else None) and a[9] == 16
    if kept:
        assert e.aux_dev["p"].nbytes == 2 * 5 * 7 * 16 * 4 and a[0] == a[1] == x.buf.ptr
    assert set(e.blobs) == {"data", "x", "out"} | ({"y"} if top == "y" else set()) | ({"target", "loss"})
    if phase == "TRAIN":
        down = "lr_mult: 0" not in front
        kinds = [(op.kind, op.name) for op in e.plan.ops if op.kind == "neuron_bwd"]
        assert kinds == ([("neuron_bwd", "p")] if down else [])
        reads_x = name.startswith(("Swish", "AbsVal"))
        for fn, a in run(e, [op for op in e.plan.ops if op.kind == "neuron_bwd"]):
            ref = (e.aux_dev["p"].ptr, 16, 0) if kept else (x.buf.ptr, x.cstride, x.coffset) if reads_x else (y.buf.ptr, y.cstride, y.coffset)
            assert fn == "fcn_neuron_bwd_f32" and (a[1], a[7], a[8]) == ref and a[-2] == 0, name


def test_the_backward_order_and_what_each_launch_reads(stub):
    e = stub(SIX + LOSS, "TRAIN")
    ops = [op for op in e.plan.ops if op.kind == "neuron_bwd"]
    assert [op.name for op in ops] == ["s", "b", "c", "r", "a", "e"]      # the file in reverse
    assert sorted(e.aux_dev) == [] or "s" not in e.aux_dev      # (s has a top of its own: its bottom c is still there)
    G, B = e.grad_blobs, e.blobs
    pix, c = 70, 16
    want = [  # (dY, ref, dX, mode, a, b): y for ELU / Clip / BNLL, x for AbsVal / Swish; in place dX is dY
        ("s", "c", "c", L.NEURON_SWISH, 1.5, 0.0), ("c", "c", "c", L.NEURON_BNLL, 0.0, 0.0), ("c", "c", "a", L.NEURON_CLIP, -1.0, 2.0),
        ("a", "a", "a", L.NEURON_CLIP, 0.0, 6.0), ("a", "x", "x", L.NEURON_ABSVAL, 0.0, 0.0), ("x", "x", "x", L.NEURON_ELU, 0.5, 0.0)]
    calls = run(e, ops)
    for (fn, a), (gy, ref, gx, mode, pa, pb) in zip(calls, want):
        assert fn == "fcn_neuron_bwd_f32"
        assert a == (G[gy].buf.ptr, B[ref].buf.ptr, G[gx].buf.ptr, pix, c, G[gy].cstride, 0, B[ref].cstride, 0, G[gx].cstride, 0, mode, pa, pb, 0, None)


def test_accumulate_follows_one_bottoms_rules(stub):
    """Not in place, the launch accumulates exactly when the view of its bottom already holds a gradient."""
    other = 'layer { name: "o" type: "Convolution" bottom: "x" top: "z" convolution_param { num_output: 16 kernel_size: 1 } }\n'
    tail = 'layer { name: "sum" type: "Eltwise" bottom: "y" bottom: "z" top: "sum" }\n' + OUT % "sum" + LOSS
    for t, body in (("ELU", ""), ("ReLU6", ""), ("Clip", "clip_param { min: 0 max: 1 }"), ("AbsVal", ""), ("BNLL", ""), ("Swish", "")):
        act = 'layer { name: "p" type: "%s" bottom: "x" top: "y" %s }\n' % (t, body)
        for layers, acc in ((act + other, 1), (other + act, 0)):      # (backward walks the file in reverse)
            e = stub(DATA + CONV + layers + tail, "TRAIN")
            assert "p" not in e.aux_dev
            (fn, a), = run(e, [op for op in e.plan.ops if op.kind == "neuron_bwd"])
            gx, gy = e.grad_blobs["x"], e.grad_blobs["y"]
            ref = e.blobs["x" if t in ("AbsVal", "Swish") else "y"]
            assert a[:3] == (gy.buf.ptr, ref.buf.ptr, gx.buf.ptr) and a[-2:] == (acc, None), (t, acc)


def test_windows_and_their_refusals_by_layer_name(stub):
    e = stub(SIX)
    p = next(l for l in e.spec.layers if l.name == "e")
    x = e.blobs["x"]
    x.coffset, x.cstride = 4, 24      # a 16-byte-aligned channel window of a wider buffer: the launch takes it as it is
    (_, a), = run(e, e._fwd_neuron(p, []))
    assert a[5:9] == (24, 4, 24, 4)
    x.coffset = 6
    with pytest.raises(NotImplementedError, match="ELU e: a channel window that is not 16-byte aligned"):
        e._fwd_neuron(p, [])
    h = stub(SIX, f16=True)
    x = h.blobs["x"]
    x.coffset, x.cstride = 4, 24      # a float32 window is none in halves: groups of 8
    with pytest.raises(NotImplementedError, match="ELU e: a channel window that is not 16-byte aligned"):
        h._fwd_neuron(p, ["x"])
    x.coffset = 8
    (fn, a), = run(h, h._fwd_neuron(p, ["x"]))
    assert fn == "fcn_neuron_fwd_f16" and a[4:8] == (24, 8, 24, 8)
    a_layer = next(l for l in h.spec.layers if l.name == "a")
    h.blobs["a"].esize = 4
    with pytest.raises(NotImplementedError, match="f16 engine: AbsVal a between half and float32 blobs"):
        h._fwd_neuron(a_layer, ["x"])
    h.blobs["a"].esize = 2
    h.blobs["a"].shape = h.blobs["x"].shape = (2, 16, 35)
    with pytest.raises(NotImplementedError, match="AbsVal a on a blob that is neither 4-d nor 2-d"):
        h._fwd_neuron(a_layer, ["x"])
    t = stub(SIX + LOSS, "TRAIN")
    t.grad_blobs["x"].coffset = 2
    t.plan.ops = []
    with pytest.raises(NotImplementedError, match="backward of ELU e: the view of x is not 16-byte aligned"):
        t.plan._neuron(p, t.grad_blobs["x"], t.grad_blobs["x"], 0)


def signature(e):
    fwd = [(type(t).__name__, t.layer.name, [(op.kind, op.name) for op in t.ops] if isinstance(t, E.OpTask) else int(t.desc.flags)) for t in e.tasks]
    bwd = [(op.kind, op.name) for op in e.plan.ops] if hasattr(e, "plan") else None
    blobs = {n: (b.buf.ptr, b.coffset, b.cstride, b.esize) for n, b in e.blobs.items()}
    return fwd, bwd, blobs, [(s.layer, s.index, s.kind, s.offset, s.count, s.esize) for s in e.param_layout], sorted(e.aux_dev)


def digest(e):
    return hashlib.sha256(repr(signature(e)).encode()).hexdigest()[:16]


# recorded on the parent commit with this file's signature(): launch lists, backward ops, blob views, parameter layout, kept copies
PARENT = {
    ("resnet", "TEST", False): "815b90ccbed24b20", ("resnet", "TRAIN", False): "d9e160e9ea23894c", ("resnet", "TEST", True): "06300265c42adde1",
    ("onet", "TEST", False): "cb1f3a44178944e1", ("pnet", "TRAIN", False): "d9e1d14878dd57d6", ("onet", "TEST", True): "5227b19139b593dd",
}


@pytest.mark.parametrize("net,phase,f16", sorted(PARENT), ids=["%s %s%s" % (n, p, " halves" if h else "") for n, p, h in sorted(PARENT)])
def test_nets_without_these_layers_plan_as_before(stub, net, phase, f16):
    ph = "DEPLOY" if phase == "TEST" else "TRAIN"
    txt = models.resnet(ph, depth=50, width_div=8, size=64, num_classes=10, batch=2) if net == "resnet" else models.mtcnn(net, ph, 2)
    e = stub(txt, phase, f16=f16)
    assert digest(e) == PARENT[(net, phase, f16)]
    assert not fwd_ops(e) and not any(op.kind == "neuron_bwd" for op in getattr(getattr(e, "plan", None), "ops", []))


SMALL = dict(width_div=4, size=64, batch=2, classes=10)


@pytest.mark.parametrize("kw", [SMALL, dict(batch=1)], ids=["width_div 4 at 64", "full width at 224"])
def test_mobilenet_v2_with_relu6_plans_completely(stub, kw):
    e = stub(models.mobilenet_v2("TRAIN", relu6=True, **kw), "TRAIN")
    six = [l.name for l in e.spec.layers if l.type == "ReLU6"]
    assert len(six) == 35 and [op.name for op in fwd_ops(e)] == six and not any(n in e.aux_dev for n in six)
    assert [op.name for op in e.plan.ops if op.kind == "neuron_bwd"] == six[::-1]
    assert all(ch.relu is None for ch in e._bn_chains.values()) and not any(m["relu"] for m in e._conv_layer_meta.values())
    h = stub(models.mobilenet_v2("DEPLOY", relu6=True, **kw), f16=True)
    assert [op.name for op in fwd_ops(h)] == six and all(h.blobs[n.replace("relu", "conv")].esize == 2 for n in six)
    calls = run(h, fwd_ops(h))
    assert {fn for fn, _a in calls} == {"fcn_neuron_fwd_f16"} and all(a[8:11] == (L.NEURON_CLIP, 0.0, 6.0) for _fn, a in calls)


@pytest.mark.parametrize("kw", [SMALL, dict(batch=1)], ids=["width_div 4 at 64", "full width at 224"])
def test_efficientnet_b0_plans_completely(stub, kw):
    e = stub(models.efficientnet_b0("TRAIN", **kw), "TRAIN")
    sw = [l.name for l in e.spec.layers if l.type == "Swish"]
    assert len(sw) == 49 and [op.name for op in fwd_ops(e)] == sw
    assert sorted(n for n in e.aux_dev if n in sw) == sorted(sw)      # in place everywhere, and a gradient comes to every one
    assert [op.name for op in e.plan.ops if op.kind == "neuron_bwd"] == sw[::-1]
    assert [op.kind for op in e.plan.ops].count("scale_gate_bwd") == 32
    for fn, a in run(e, [op for op in e.plan.ops if op.kind == "neuron_bwd"]):
        assert a[11] == L.NEURON_SWISH and a[12] == 1.0 and a[-2] == 0 and a[0] == a[2]      # in place: dX is dY, never accumulating
    refs = {a[1] for _fn, a in e.fake.calls}
    assert refs == {e.aux_dev[n].ptr for n in sw}      # every gradient launch reads its kept copy
    h = stub(models.efficientnet_b0("DEPLOY", **kw), f16=True)      # halves: the whole net, the gates (tops of a Sigmoid) float32
    assert [op.name for op in fwd_ops(h)] == sw and not h.aux_dev
    assert all(h.blobs[l.tops[0]].esize == 4 for l in h.spec.layers if l.type == "Sigmoid")
    assert all(h.blobs[l.tops[0]].esize == 2 for l in h.spec.layers if l.type == "Swish")
    assert [op.kind for t in h.tasks if isinstance(t, E.OpTask) for op in t.ops].count("scale_gate") == 16
