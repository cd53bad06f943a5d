"""PReLU, TanH and Bias (csrc/act.hip) as the forward and backward planners lay them out - without a GPU.

The stub engine of tests/plan_stub.py (a NetSpec built by NetSpec.public's rule, so with activations=True): Engine / TrainEngine /
BackwardPlanner methods run with DeviceBuffer replaced by a counter of addresses and the library by one whose entry points return 0
(size queries: 64).  Checked:
one launch per layer and its operands in both element types; a convolution's or a BatchNorm chain's fusion ends in front of a PReLU; the
kept copy exists exactly where a gradient comes to an in-place PReLU; windows and the refusals by layer name; the parameter-gradient
launch before the data launch, each left out where nothing wants it; that a ResNet - a net without one of the three layers - has the
same launch lists and storage plans with and without the keyword; and that models.mtcnn and models.enet plan completely."""
import pytest

from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import models
from fcn_object_detector_amd import storage as S
from plan_stub import engine_factory


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, public=True)


def fwd_ops(e, kinds=("act",)):
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
THREE = (DATA + CONV + 'layer { name: "p" type: "PReLU" bottom: "x" top: "x" }\n'
         'layer { name: "t" type: "TanH" bottom: "x" top: "t" }\n'
         'layer { name: "b" type: "Bias" bottom: "t" top: "t" }\n'
         'layer { name: "s" type: "PReLU" bottom: "t" top: "s" prelu_param { channel_shared: true } }\n' + OUT % "s")


@pytest.mark.parametrize("f16", [False, True])
def test_one_launch_per_layer_in_both_element_types(stub, f16):
    e = stub(THREE, f16=f16)
    ops = fwd_ops(e)
    assert [op.name for op in ops] == ["p", "t", "b", "s"]
    B, P = e.blobs, e.params_dev
    x, t, s = B["x"], B["t"], B["s"]
    assert all(b.esize == (2 if f16 else 4) for b in (x, t, s)) and B["out"].esize == 4      # halves in, halves out; the net's output float32
    calls = run(e, ops)
    pix, c = 2 * 5 * 7, 16
    if f16:
        assert calls == [
            ("fcn_act_fwd_f16", (x.buf.ptr, x.buf.ptr, pix, c, x.cstride, x.coffset, x.cstride, x.coffset, L.ACT_PRELU, P["p"][0].ptr, 0, None)),
            ("fcn_act_fwd_f16", (x.buf.ptr, t.buf.ptr, pix, c, x.cstride, x.coffset, t.cstride, t.coffset, L.ACT_TANH, None, 0, None)),
            ("fcn_act_fwd_f16", (t.buf.ptr, t.buf.ptr, pix, c, t.cstride, t.coffset, t.cstride, t.coffset, L.ACT_BIAS, P["b"][0].ptr, 0, None)),
            ("fcn_act_fwd_f16", (t.buf.ptr, s.buf.ptr, pix, c, t.cstride, t.coffset, s.cstride, s.coffset, L.ACT_PRELU, P["s"][0].ptr, 1, None))]
    else:
        assert calls == [
            ("fcn_act_fwd_f32", (x.buf.ptr, x.buf.ptr, None, pix, c, x.cstride, 0, x.cstride, 0, 16, L.ACT_PRELU, P["p"][0].ptr, 0, None)),
            ("fcn_act_fwd_f32", (x.buf.ptr, t.buf.ptr, None, pix, c, x.cstride, 0, t.cstride, 0, 16, L.ACT_TANH, None, 0, None)),
            ("fcn_act_fwd_f32", (t.buf.ptr, t.buf.ptr, None, pix, c, t.cstride, 0, t.cstride, 0, 16, L.ACT_BIAS, P["b"][0].ptr, 0, None)),
            ("fcn_act_fwd_f32", (t.buf.ptr, s.buf.ptr, None, pix, c, t.cstride, 0, s.cstride, 0, 16, L.ACT_PRELU, P["s"][0].ptr, 1, None))]
    assert not e.aux_dev      # (a TEST engine keeps nothing)
    # the parameters are float32 in both engines: PLAIN segments of 4-byte elements
    assert all(seg.esize == 4 and seg.kind == S.PLAIN for seg in e.param_layout if seg.layer in ("p", "b", "s"))


def test_without_the_keyword_the_engines_refuse_tanh_as_before(stub):
    tanh = DATA + CONV + 'layer { name: "t" type: "TanH" bottom: "x" top: "x" }\n' + OUT % "x"
    with pytest.raises(NotImplementedError, match="layer type 'TanH' .layer t. has no forward kernel yet"):
        stub(tanh, activations=False)
    with pytest.raises(NotImplementedError, match="f16 engine: layer type TanH .t. has no half-float kernel"):
        stub(tanh, activations=False, f16=True)
    assert [op.name for op in fwd_ops(stub(tanh))] == ["t"] and [op.name for op in fwd_ops(stub(tanh, f16=True))] == ["t"]


def test_a_float32_net_output_of_one_of_them_stays_refused_in_halves(stub):
    for layer in ('layer { name: "p" type: "PReLU" bottom: "x" top: "y" }', 'layer { name: "p" type: "TanH" bottom: "x" top: "y" }',
                  'layer { name: "p" type: "Bias" bottom: "x" top: "y" }'):
        with pytest.raises(NotImplementedError, match="f16 engine: float32 blob y is produced by"):
            stub(DATA + CONV + layer, f16=True)
        assert [op.name for op in fwd_ops(stub(DATA + CONV + layer))] == ["p"]      # (float32: nothing to refuse)


def test_a_fusion_ends_in_front_of_a_prelu(stub):
    """As in front of a ReLU with a slope: the convolution epilogue and the BatchNorm chain recognise only a plain ReLU."""
    e = stub(DATA + CONV + 'layer { name: "p" type: "PReLU" bottom: "x" top: "x" }\n' + OUT % "x")
    assert not e._conv_layer_meta["x"]["relu"] and not (e._conv_flags["x"] & L.CONV_RELU) and [op.name for op in fwd_ops(e)] == ["p"]
    relu = stub(DATA + CONV + 'layer { name: "p" type: "ReLU" bottom: "x" top: "x" }\n' + OUT % "x")
    assert relu._conv_layer_meta["x"]["relu"] and relu._conv_flags["x"] & L.CONV_RELU and not fwd_ops(relu, ("act", "relu"))
    chain = (DATA + CONV + 'layer { name: "bn" type: "BatchNorm" bottom: "x" top: "x" }\n'
             'layer { name: "sc" type: "Scale" bottom: "x" top: "x" scale_param { bias_term: true } }\n'
             'layer { name: "p" type: "PReLU" bottom: "x" top: "x" }\n' + OUT % "x")
    e = stub(chain)
    ch = e._bn_chains["bn"]
    assert ch.scale is not None and ch.relu is None
    assert [(op.kind, op.name) for op in fwd_ops(e, ("bn_apply", "act", "relu"))] == [("bn_apply", "bn+sc"), ("act", "p")]
    (_, a), = run(e, fwd_ops(e, ("bn_apply",)))
    assert a[-2] == 0      # (the apply launch's relu flag)
    e = stub(DATA + 'layer { name: "ip" type: "InnerProduct" bottom: "data" top: "ip" inner_product_param { num_output: 12 } }\n'
             'layer { name: "p" type: "PReLU" bottom: "ip" top: "ip" }\n')
    assert not e._conv_layer_meta["ip"]["relu"] and [op.name for op in fwd_ops(e)] == ["p"]
    (_, a), = run(e, fwd_ops(e))
    assert a[3:5] == (2, 12)      # a 2-d blob: N pixels of C channels


KEEP_CASES = [
    # (name, the PReLU layer, layers in front, phase, kept?)
    ("in place, TRAIN, a gradient comes", 'layer { name: "p" type: "PReLU" bottom: "x" top: "x" }', CONV, "TRAIN", True),
    ("in place, TRAIN, frozen slopes, the bottom needs a gradient", 'layer { name: "p" type: "PReLU" bottom: "x" top: "x" param { lr_mult: 0 } }', CONV, "TRAIN", True),
    ("in place, TRAIN, slopes learn, the bottom needs none", 'layer { name: "p" type: "PReLU" bottom: "x" top: "x" }',
     FROZEN, "TRAIN", True),
    ("in place, TRAIN, nothing in front or in it learns", 'layer { name: "p" type: "PReLU" bottom: "x" top: "x" param { lr_mult: 0 } }',
     FROZEN, "TRAIN", False),
    ("a top of its own, TRAIN", 'layer { name: "p" type: "PReLU" bottom: "x" top: "y" }', CONV, "TRAIN", False),
    ("in place, TEST", 'layer { name: "p" type: "PReLU" bottom: "x" top: "x" }', CONV, "TEST", False),
]


@pytest.mark.parametrize("name,layer,front,phase,kept", KEEP_CASES, ids=[c[0] for c in KEEP_CASES])
def test_the_kept_copy_is_there_exactly_when_needed(stub, name, layer, front, phase, kept):
    top = "y" if 'top: "y"' in layer else "x"
    e = stub(DATA + front + layer + "\n" + OUT % top + LOSS, phase)
    assert ("p" in e.aux_dev) == kept
    (fn, a), = run(e, fwd_ops(e))
    x = e.blobs["x"]
    assert fn == "fcn_act_fwd_f32" and a[2] == (e.aux_dev["p"].ptr if kept else None) and a[9] == 16
    if kept:
        assert e.aux_dev["p"].nbytes == 2 * 5 * 7 * 16 * 4 and a[0] == a[1] == x.buf.ptr
    # nothing else changes: no blob is renamed or un-aliased, the in-place layer still writes its bottom's buffer
    assert set(e.blobs) == {"data", "x", "out"} | ({"y"} if top == "y" else set()) | ({"target", "loss"})
    if phase == "TRAIN":
        kinds = [(op.kind, op.name) for op in e.plan.ops if op.kind.startswith("act_bwd")]
        learns, down = "lr_mult: 0" not in layer, "lr_mult: 0" not in front
        assert kinds == ([("act_bwd_param", "p")] if learns else []) + ([("act_bwd", "p")] if down or learns else [])
        for fn, a in run(e, [op for op in e.plan.ops if op.kind.startswith("act_bwd")]):
            ref = (e.aux_dev["p"].ptr, 16, 0) if kept else (x.buf.ptr, x.cstride, x.coffset)      # the kept copy, or the bottom itself
            assert (a[1], a[7], a[8]) == ref, fn


def test_the_parameter_gradient_comes_first_and_both_read_the_kept_copy(stub):
    e = stub(DATA + CONV + 'layer { name: "p" type: "PReLU" bottom: "x" top: "x" }\n'
             'layer { name: "b" type: "Bias" bottom: "x" top: "x" }\nlayer { name: "t" type: "TanH" bottom: "x" top: "x" }\n' + OUT % "x" + LOSS, "TRAIN")
    ops = [op for op in e.plan.ops if op.kind.startswith("act_bwd")]
    assert [(op.kind, op.name) for op in ops] == [("act_bwd", "t"), ("act_bwd_param", "b"), ("act_bwd", "b"), ("act_bwd_param", "p"), ("act_bwd", "p")]
    assert [getattr(op, "layers", None) for op in ops] == [None, ["b"], None, ["p"], None]      # (what the gradient exchange waits for)
    g, x, keep, pix, c = e.grad_blobs["x"], e.blobs["x"], e.aux_dev["p"], 70, 16
    dp, db = e._grad_view("p", 0).ptr, e._grad_view("b", 0).ptr
    assert dp != db and e.plan.act_ws is not None and e.plan.act_ws.nbytes == 64
    calls = run(e, ops)
    assert calls == [
        # in place: dX is dY and never accumulates; TanH reads its OUTPUT, the blob itself
        ("fcn_act_bwd_data_f32", (g.buf.ptr, x.buf.ptr, g.buf.ptr, pix, c, g.cstride, 0, x.cstride, 0, g.cstride, 0, L.ACT_TANH, None, 0, 0, None)),
        ("fcn_act_bwd_param_f32", (g.buf.ptr, None, db, pix, c, g.cstride, 0, 0, 0, L.ACT_BIAS, 0, e._act_ws.ptr, None)),
        ("fcn_act_bwd_data_f32", (g.buf.ptr, None, g.buf.ptr, pix, c, g.cstride, 0, 0, 0, g.cstride, 0, L.ACT_BIAS, None, 0, 0, None)),
        ("fcn_act_bwd_param_f32", (g.buf.ptr, keep.ptr, dp, pix, c, g.cstride, 0, 16, 0, L.ACT_PRELU, 0, e._act_ws.ptr, None)),
        ("fcn_act_bwd_data_f32", (g.buf.ptr, keep.ptr, g.buf.ptr, pix, c, g.cstride, 0, 16, 0, g.cstride, 0, L.ACT_PRELU, e.params_dev["p"][0].ptr, 0, 0,
                                  None))]


def test_accumulate_follows_one_bottoms_rules(stub):
    """Not in place, the launch accumulates exactly when the view of its bottom already holds a gradient."""
    other = 'layer { name: "o" type: "Convolution" bottom: "x" top: "z" convolution_param { num_output: 16 kernel_size: 1 } }\n'
    act = 'layer { name: "p" type: "PReLU" bottom: "x" top: "y" prelu_param { channel_shared: true } }\n'
    tail = 'layer { name: "sum" type: "Eltwise" bottom: "y" bottom: "z" top: "sum" }\n' + OUT % "sum" + LOSS
    for layers, acc in ((act + other, 1), (other + act, 0)):      # (backward walks the file in reverse)
        e = stub(DATA + CONV + layers + tail, "TRAIN")
        assert "p" not in e.aux_dev
        calls = run(e, [op for op in e.plan.ops if op.kind.startswith("act_bwd")])
        assert [fn for fn, _a in calls] == ["fcn_act_bwd_param_f32", "fcn_act_bwd_data_f32"]
        (_, ap), (_, ad) = calls
        gx, gy, x = e.grad_blobs["x"], e.grad_blobs["y"], e.blobs["x"]
        assert ap[:3] == (gy.buf.ptr, x.buf.ptr, e._grad_view("p", 0).ptr) and ap[10] == 1      # the shared slope: one value
        assert ad[:3] == (gy.buf.ptr, x.buf.ptr, gx.buf.ptr) and ad[-4:] == (e.params_dev["p"][0].ptr, 1, acc, None)


def test_windows_and_their_refusals_by_layer_name(stub):
    e = stub(THREE)
    p = next(l for l in e.spec.layers if l.name == "p")
    x = e.blobs["x"]
    x.coffset, x.cstride = 4, 24      # a 16-byte-aligned channel window of a wider buffer: the launch takes it as it is
    (_, a), = run(e, e._fwd_act(p, []))
    assert a[5:9] == (24, 4, 24, 4)
    x.coffset = 6
    with pytest.raises(NotImplementedError, match="PReLU p: a channel window that is not 16-byte aligned"):
        e._fwd_act(p, [])
    h = stub(THREE, f16=True)
    x = h.blobs["x"]
    x.coffset, x.cstride = 4, 24      # a float32 window is none in halves: groups of 8
    with pytest.raises(NotImplementedError, match="PReLU p: a channel window that is not 16-byte aligned"):
        h._fwd_act(p, ["x"])
    x.coffset = 8
    (fn, a), = run(h, h._fwd_act(p, ["x"]))
    assert fn == "fcn_act_fwd_f16" and a[4:8] == (24, 8, 24, 8)


def signature(e):
    fwd = [(type(t).__name__, t.layer.name, [(op.kind, op.name) for op in t.ops] if isinstance(t, E.OpTask) else int(t.desc.flags)) for t in e.tasks]
    bwd = [(op.kind, op.name) for op in e.plan.ops] if hasattr(e, "plan") else None
    blobs = {n: (b.buf.ptr, b.coffset, b.cstride, b.esize) for n, b in e.blobs.items()}
    return fwd, bwd, blobs, [(s.layer, s.index, s.kind, s.offset, s.count, s.esize) for s in e.param_layout], sorted(e.aux_dev)


@pytest.mark.parametrize("phase,f16", [("TEST", False), ("TRAIN", False), ("TEST", True)], ids=["f32 TEST", "f32 TRAIN", "halves"])
def test_a_resnet_plans_identically_with_and_without_the_keyword(stub, phase, f16):
    txt = models.resnet("DEPLOY" if phase == "TEST" else "TRAIN", depth=50, width_div=8, size=64, num_classes=10, batch=2)
    a, b = signature(stub(txt, phase, f16=f16, activations=False)), signature(stub(txt, phase, f16=f16, activations=True))
    assert a == b and len(a[0]) > 50 and not any(k == "act" for _t, _n, ops in a[0] if isinstance(ops, list) for k, _ in ops)


@pytest.mark.parametrize("net", ["pnet", "rnet", "onet"])
def test_mtcnn_plans_completely(stub, net):
    n_act = {"pnet": 3, "rnet": 4, "onet": 5}[net]
    e = stub(models.mtcnn(net, "DEPLOY", 2))
    assert len(fwd_ops(e)) == n_act and not e.aux_dev
    e = stub(models.mtcnn(net, "TRAIN", 2), "TRAIN")
    acts = [l.name for l in e.spec.layers if l.type == "PReLU"]
    assert sorted(n for n in e.aux_dev if n in acts) == sorted(acts)      # in place everywhere, and everything learns
    kinds = [(op.kind, op.name) for op in e.plan.ops if op.kind.startswith("act_bwd")]
    assert kinds == [(k, n) for n in reversed(acts) for k in ("act_bwd_param", "act_bwd")]
    if net == "pnet":      # fully convolutional: another size plans alike
        assert len(fwd_ops(stub(models.mtcnn("pnet", "DEPLOY", 2, size=(33, 47))))) == 3
        with pytest.raises(NotImplementedError, match="f16 engine: MAX pooling pool1 over 10 channels"):
            stub(models.mtcnn("pnet", "DEPLOY", 2), f16=True)
    if net == "onet":      # 32 / 64 / 64 / 128 channels: the half-float engine takes it
        h = stub(models.mtcnn("onet", "DEPLOY", 2), f16=True)
        assert len(fwd_ops(h)) == 5 and all(h.blobs[l.tops[0]].esize == 2 for l in h.spec.layers if l.type == "PReLU")


def test_enet_plans_completely(stub):
    kw = dict(classes=5, batch=2, size=(32, 64), width_div=4)
    e = stub(models.enet("DEPLOY", **kw))
    n_prelu = sum(l.type == "PReLU" for l in e.spec.layers)
    assert n_prelu == 82 and len(fwd_ops(e)) == n_prelu
    chains = [ch for ch in e._bn_chains.values()]
    assert len(chains) == 1 + 27 * 3 + 4 and all(ch.relu is None for ch in chains)      # every chain ends in front of its PReLU
    e = stub(models.enet("TRAIN", **kw), "TRAIN")
    acts = [l.name for l in e.spec.layers if l.type == "PReLU"]
    assert all(n in e.aux_dev for n in acts)
    kinds = [(op.kind, op.name) for op in e.plan.ops if op.kind.startswith("act_bwd")]
    assert kinds == [(k, n) for n in reversed(acts) for k in ("act_bwd_param", "act_bwd")]
    assert [op.name for op in e.plan.ops if op.kind == "unpool_bwd"] == ["b5_0/unpool", "b4_0/unpool"]
    full = stub(models.enet("TEST"))
    assert full.blobs["fullconv"].shape == (1, 19, 512, 1024) and len(fwd_ops(full)) == n_prelu
    with pytest.raises(NotImplementedError, match="f16 engine: pooling initial/pool"):      # (the image is float32: README says so)
        stub(models.enet("DEPLOY", **kw), f16=True)
