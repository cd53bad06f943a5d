"""ShuffleChannel (csrc/shuffle.hip) as the forward and backward planners lay it out - without a GPU.

The stub engine of tests/plan_stub.py, on a bare NetSpec and on NetSpec.public's alike (the layer needs no keyword).  Checked: one
`shuffle` op per layer and its arguments in both element types; the top owns its buffer - never a window of the bottom, never the target
a Concat member is written into through it; a stride-1 unit of ShuffleNet v2 plans as Slice views -> branch -> Concat -> one shuffle
launch; the backward launch uses group C / g and the accumulate flag in both states; windows and the refusals by layer name; the
half-float plan of models.shufflenet_v2(width=0.5) goes through to prob, and models.shufflenet_v1 is refused in halves at its first
grouped convolution by layer name; and ResNet-50, MobileNet-v2 and EfficientNet-B0 - nets without the layer - plan launch for launch and
argument for argument as they do with the shuffle tables emptied."""
import pytest

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import models
from plan_stub import engine_factory


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, public=True)


@pytest.fixture
def bare(monkeypatch):
    return engine_factory(monkeypatch)


def fwd_ops(e, kinds=("shuffle",)):
    return [op for t in e.tasks if isinstance(t, E.OpTask) for op in t.ops if op.kind in kinds]


def run(e, ops):
    del e.fake.calls[:]
    for op in ops:
        op.run(None)
    return list(e.fake.calls)


DATA = 'layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 2 dim: 8 dim: 5 dim: 7 } } }\n'
CONV = 'layer { name: "x" type: "Convolution" bottom: "data" top: "x" convolution_param { num_output: 24 kernel_size: 3 pad: 1 } }\n'
SH = 'layer { name: "%s" type: "ShuffleChannel" bottom: "%s" top: "%s" shuffle_channel_param { group: %d } }\n'
OUT = 'layer { name: "out" type: "Convolution" bottom: "%s" top: "out" convolution_param { num_output: 8 kernel_size: 1 } }\n'
LOSS = ('layer { name: "target" type: "Input" top: "target" input_param { shape { dim: 2 dim: 8 dim: 5 dim: 7 } } }\n'
        'layer { name: "loss" type: "EuclideanLoss" bottom: "out" bottom: "target" top: "loss" }\n')
TWO = DATA + CONV + SH % ("s1", "x", "y", 3) + SH % ("s2", "y", "z", 4) + OUT % "z"


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("public", [False, True])
def test_one_launch_per_layer_in_both_element_types(stub, bare, f16, public):
    e = (stub if public else bare)(TWO, f16=f16)
    ops = fwd_ops(e)
    assert [op.name for op in ops] == ["s1", "s2"]
    B = e.blobs
    assert all(B[n].esize == (2 if f16 else 4) for n in ("x", "y", "z")) and B["out"].esize == 4      # halves in, halves out; the output float32
    pix, c = 2 * 5 * 7, 24
    assert all(op.bytes == 2.0 * B["x"].esize * pix * c and op.flops == 0.0 for op in ops)
    for (fn, args), (name, bot, top, g) in zip(run(e, ops), (("s1", "x", "y", 3), ("s2", "y", "z", 4))):
        x, y = B[bot], B[top]
        if f16:
            assert (fn, args) == ("fcn_shuffle_channel_f16", (x.buf.ptr, y.buf.ptr, pix, c, g, x.cstride, x.coffset, y.cstride, y.coffset, None)), name
        else:
            assert (fn, args) == ("fcn_shuffle_channel_f32", (x.buf.ptr, y.buf.ptr, pix, c, g, 24, 0, 24, 0, 0, None)), name
    assert not e.aux_dev and not any(n in e.params_dev for n in ("s1", "s2"))      # nothing kept, no blobs


def test_a_2d_blob_is_n_pixels(stub):
    e = stub(DATA + 'layer { name: "ip" type: "InnerProduct" bottom: "data" top: "ip" inner_product_param { num_output: 12 } }\n' + SH % ("s", "ip", "y", 3)
             + 'layer { name: "fc" type: "InnerProduct" bottom: "y" top: "fc" inner_product_param { num_output: 4 } }\n')
    (fn, a), = run(e, fwd_ops(e))
    assert fn == "fcn_shuffle_channel_f32" and a[2:5] == (2, 12, 3)


def test_the_top_owns_its_storage(stub):
    """Never a window of its bottom; and a Concat that reads the top copies it - the shuffle does not write into the Concat's buffer."""
    cat = (DATA + CONV + SH % ("s1", "x", "y", 3)
           + 'layer { name: "w" type: "Convolution" bottom: "data" top: "w" convolution_param { num_output: 8 kernel_size: 1 } }\n'
           'layer { name: "cat" type: "Concat" bottom: "y" bottom: "w" top: "cat" }\n' + OUT % "cat")
    for f16 in (False, True):
        e = stub(cat, f16=f16)
        B = e.blobs
        assert "y" not in e.alias and B["y"].buf is not B["x"].buf and B["y"].buf is not B["cat"].buf and B["y"].coffset == 0
        assert "cat" in e.copy_concats and B["w"].buf is not B["cat"].buf      # (one member that cannot be a view makes the whole Concat copy)
        (fn, a), = run(e, fwd_ops(e))
        assert a[1] == B["y"].buf.ptr and a[0] == B["x"].buf.ptr
        assert [op.name for op in fwd_ops(e, ("copy",))] == ["cat:y", "cat:w"]
    e = stub(TWO)
    ptrs = {e.blobs[n].buf.ptr for n in ("x", "y", "z")}
    assert len(ptrs) == 3


def test_a_float32_net_output_of_the_layer_stays_refused_in_halves(stub):
    net = DATA + CONV + SH % ("s", "x", "y", 3)
    with pytest.raises(NotImplementedError, match="f16 engine: float32 blob y is produced by"):
        stub(net, f16=True)
    assert [op.name for op in fwd_ops(stub(net))] == ["s"]      # (float32: nothing to refuse)


def test_windows_and_their_refusals_by_layer_name(stub):
    e = stub(TWO)
    s1 = next(l for l in e.spec.layers if l.name == "s1")
    x = e.blobs["x"]
    x.coffset, x.cstride = 4, 32      # a 16-byte-aligned channel window of a wider buffer: the launch takes it as it is
    (_, a), = run(e, e._fwd_shuffle(s1, []))
    assert a[5:9] == (32, 4, 24, 0)
    x.coffset = 6
    with pytest.raises(NotImplementedError, match="ShuffleChannel s1: a channel window that is not 16-byte aligned"):
        e._fwd_shuffle(s1, [])
    h = stub(TWO, f16=True)
    x = h.blobs["x"]
    x.coffset, x.cstride = 4, 32      # a float32 window is none in halves: groups of 8
    with pytest.raises(NotImplementedError, match="ShuffleChannel s1: a channel window that is not 16-byte aligned"):
        h._fwd_shuffle(s1, ["x"])
    x.coffset = 8
    (fn, a), = run(h, h._fwd_shuffle(s1, ["x"]))
    assert fn == "fcn_shuffle_channel_f16" and a[5:9] == (32, 8, 24, 0)
    h.blobs["y"].esize = 4
    with pytest.raises(NotImplementedError, match="f16 engine: ShuffleChannel s1 between half and float32 blobs"):
        h._fwd_shuffle(s1, ["x"])
    h.blobs["y"].esize = 2
    h.blobs["y"].shape = h.blobs["x"].shape = (2, 24, 35)
    with pytest.raises(NotImplementedError, match="ShuffleChannel s1 on a blob that is neither 4-d nor 2-d"):
        h._fwd_shuffle(s1, ["x"])
    t = stub(TWO + LOSS, "TRAIN")
    t.grad_blobs["x"].coffset = 2
    t.plan.ops = []
    with pytest.raises(NotImplementedError, match="backward of ShuffleChannel s1: the view of x is not 16-byte aligned"):
        t.plan._shuffle(s1, t.grad_blobs["y"], t.grad_blobs["x"], 0)


def test_the_backward_launch_uses_group_c_over_g(stub):
    e = stub(TWO + LOSS, "TRAIN")
    ops = [op for op in e.plan.ops if op.kind == "shuffle_bwd"]
    assert [op.name for op in ops] == ["s2", "s1"]      # the file in reverse
    G = e.grad_blobs
    pix, c = 70, 24
    assert all(op.bytes == 8.0 * pix * c for op in ops)
    for (fn, a), (gy, gx, g) in zip(run(e, ops), (("z", "y", 4), ("y", "x", 3))):
        assert fn == "fcn_shuffle_channel_f32"
        assert a == (G[gy].buf.ptr, G[gx].buf.ptr, pix, c, c // g, G[gy].cstride, 0, G[gx].cstride, 0, 0, None)
    assert G["y"].buf is not G["x"].buf and not e.aux_dev


def test_accumulate_follows_one_bottoms_rules(stub):
    """The launch accumulates exactly when the view of its bottom already holds a gradient."""
    other = 'layer { name: "o" type: "Convolution" bottom: "x" top: "w" convolution_param { num_output: 24 kernel_size: 1 } }\n'
    tail = 'layer { name: "sum" type: "Eltwise" bottom: "y" bottom: "w" top: "sum" }\n' + OUT % "sum" + LOSS
    sh = SH % ("p", "x", "y", 3)
    for layers, acc in ((sh + other, 1), (other + sh, 0)):      # (backward walks the file in reverse)
        e = stub(DATA + CONV + layers + tail, "TRAIN")
        op, = [op for op in e.plan.ops if op.kind == "shuffle_bwd"]
        (fn, a), = run(e, [op])
        gx, gy = e.grad_blobs["x"], e.grad_blobs["y"]
        assert a[:2] == (gy.buf.ptr, gx.buf.ptr) and a[4] == 8 and a[-2:] == (acc, None), acc
        assert op.bytes == 4.0 * (2 + acc) * 70 * 24
    frozen = CONV.replace('top: "x" ', 'top: "x" param { lr_mult: 0 } param { lr_mult: 0 } ')
    e = stub(DATA + frozen + sh + OUT % "y" + LOSS, "TRAIN")      # nothing in front learns: no gradient launch
    assert not [op for op in e.plan.ops if op.kind == "shuffle_bwd"] and [op.name for op in fwd_ops(e)] == ["p"]


def test_a_v2_unit_plans_as_slice_views_branch_concat_and_one_shuffle(stub):
    e = stub(models.shufflenet_v2("TRAIN", width_div=3, size=64, batch=2, classes=10), "TRAIN")
    B, u = e.blobs, "stage2_2"
    x = B["stage2_1/shuffle"]
    left, right = B[u + "/left"], B[u + "/right"]
    assert u + "/slice" not in e.copy_slices                                       # the Slice tops are windows of the unit's input ...
    assert left.buf is x.buf and right.buf is x.buf and (left.coffset, right.coffset) == (0, 8) and left.cstride == right.cstride == 16
    assert u + "/concat" in e.copy_concats and B[u + "/concat"].buf is not x.buf   # ... the Concat copies (its left member is such a window) ...
    assert [op.name for op in fwd_ops(e, ("copy",)) if op.name.startswith(u + "/")] == [u + "/concat:" + u + "/left", u + "/concat:" + u + "/conv2"]
    sh = B[u + "/shuffle"]
    assert sh.buf is not B[u + "/concat"].buf and u + "/shuffle" not in e.alias     # ... and the shuffle's top owns its buffer
    names = [op.name for op in fwd_ops(e)]
    assert len(names) == 16 and names.count(u + "/shuffle") == 1
    order = [(op.kind, op.name) for t in e.tasks if isinstance(t, E.OpTask) for op in t.ops if op.name.startswith(u + "/") and op.kind in ("copy", "shuffle")]
    assert [k for k, _n in order] == ["copy", "copy", "shuffle"] and order[-1] == ("shuffle", u + "/shuffle")
    bwd = [op.name for op in e.plan.ops if op.kind == "shuffle_bwd"]
    assert bwd == names[::-1]
    calls = run(e, [op for op in e.plan.ops if op.kind == "shuffle_bwd"])
    assert all(a[4] == a[3] // 2 and a[-2] == 0 for _fn, a in calls)      # group C / 2; each unit's Concat gradient has one writer


def test_shufflenet_v1_plans_completely_in_float32(stub):
    e = stub(models.shufflenet_v1("TRAIN", width_div=5, size=64, batch=2, classes=10), "TRAIN")
    names = ["shuffle%d" % i for i in range(1, 17)]
    assert [op.name for op in fwd_ops(e)] == names and [op.name for op in e.plan.ops if op.kind == "shuffle_bwd"] == names[::-1]
    calls = run(e, fwd_ops(e))
    assert all(fn == "fcn_shuffle_channel_f32" and a[4] == 3 and a[3] % 12 == 0 for fn, a in calls)
    calls = run(e, [op for op in e.plan.ops if op.kind == "shuffle_bwd"])
    assert all(a[4] == a[3] // 3 and a[-2] == 0 for _fn, a in calls)
    full = stub(models.shufflenet_v1("TRAIN", batch=1), "TRAIN")
    assert [a[3] for _fn, a in run(full, fwd_ops(full))] == [60] * 4 + [120] * 8 + [240] * 4


@pytest.mark.parametrize("kw", [dict(width_div=3, size=64, batch=2, classes=10), dict(batch=1), dict(batch=1, width=1.5)],
                         ids=["width_div 3 at 64", "0.5x at 224", "1.5x at 224"])
def test_shufflenet_v2_in_halves_goes_through_to_prob(stub, kw):
    h = stub(models.shufflenet_v2("DEPLOY", **kw), f16=True)
    ops = fwd_ops(h)
    assert len(ops) == 16 and {fn for fn, _a in run(h, ops)} == {"fcn_shuffle_channel_f16"}
    assert all(h.blobs[l.tops[0]].esize == h.blobs[l.bottoms[0]].esize == 2 for l in h.spec.layers if l.type == "ShuffleChannel")
    assert h.blobs["prob"].esize == 4 and h.spec.output_blobs() == ["prob"]
    assert [op.kind for t in h.tasks if isinstance(t, E.OpTask) for op in t.ops][-1] == "softmax"
    assert all(h.blobs[l.tops[0]].coffset % 8 == 0 for l in h.spec.layers if l.type == "Slice")      # every branch a window on 16 bytes of halves


def test_shufflenet_v1_is_refused_in_halves_at_its_first_grouped_convolution(stub):
    with pytest.raises(NotImplementedError, match="grouped Convolution resx1_conv3: group 3 leaves 20 input and 72 output channels per group, "
                                                  r"not whole 16-byte segments \(8 halves\)"):
        stub(models.shufflenet_v1("DEPLOY"), f16=True)


# ---------------------------------------------------------------------------------------------------------------- what must not move
def everything(e):
    """Storage, forward tasks, backward launches and the ordered (name, args) of every library call made by running each launch once."""
    fwd = [(type(t).__name__, t.layer.name, [(op.kind, op.name, op.flops, op.bytes) for op in t.ops] if isinstance(t, E.OpTask) else int(t.desc.flags))
           for t in e.tasks]
    bwd = [(op.kind, op.name, op.flops, op.bytes) for op in e.plan.ops] if hasattr(e, "plan") else None
    blobs = {n: (b.buf.ptr, b.coffset, b.cstride, b.esize) for n, b in e.blobs.items()}
    layout = [(s.layer, s.index, s.kind, s.offset, s.count, s.esize) for s in e.param_layout]
    calls = run(e, [op for t in e.tasks if isinstance(t, E.OpTask) for op in t.ops] + (list(e.plan.ops) if hasattr(e, "plan") else []))
    plain = lambda v: v if v is None or isinstance(v, (int, float, str)) else type(v).__name__      # (a descriptor passed by reference: its type)
    return fwd, bwd, blobs, layout, sorted(e.aux_dev), [(fn, tuple(plain(v) for v in a)) for fn, a in calls]


NETS = {"resnet50": lambda ph: models.resnet(ph, depth=50, width_div=8, size=64, num_classes=10, batch=2),
        "mobilenet_v2": lambda ph: models.mobilenet_v2(ph, width_div=4, size=64, batch=2, classes=10),
        "efficientnet_b0": lambda ph: models.efficientnet_b0(ph, width_div=4, size=64, batch=2, classes=10)}


@pytest.mark.parametrize("phase,f16", [("TEST", False), ("TRAIN", False), ("TEST", True)], ids=["TEST", "TRAIN", "TEST halves"])
@pytest.mark.parametrize("net", sorted(NETS))
def test_nets_without_the_layer_plan_as_with_the_shuffle_tables_emptied(stub, monkeypatch, net, phase, f16):
    txt = NETS[net]("DEPLOY" if phase == "TEST" else "TRAIN")
    now = everything(stub(txt, phase, f16=f16))
    assert not any(fn.startswith("fcn_shuffle") for fn, _a in now[-1]) and len(now[-1]) > 50
    with monkeypatch.context() as m:
        m.setattr(E, "SHUFFLE_TYPES", ())
        m.setattr(BW, "SHUFFLE_TYPES", ())
        emptied = stub(txt, phase, f16=f16)
        if phase == "TRAIN":
            assert emptied.plan.shuffles == {}
        assert everything(emptied) == now
    t = stub(TWO + LOSS, "TRAIN")      # (and the table is what makes the layer plan)
    assert set(t.plan.shuffles) == {"ShuffleChannel"}
