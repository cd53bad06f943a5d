"""Dilated and rectangular Convolution as the half-float forward planner lays them out - without a GPU.

The stub engine of tests/plan_stub.py (DeviceBuffer a counter of addresses, the library one whose every entry point returns 0), here a
half-float one over a bare NetSpec built with rconv_f16=True: the arithmetic of the descriptors over halves, which launches share a plan
and that the half entry points are the ones called, every refusal by layer name, that a bare NetSpec refuses as it always did, that the
float32 plan of the same nets does not depend on the keyword, and that the model writers' nets plan completely."""
import pytest

from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import NetSpec
from plan_stub import engine_factory
from test_rect_plan import FILL, one, plan_signature

NET = """
input: "data" input_shape { dim: 2 dim: 3 dim: 12 dim: 14 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 6 kernel_size: 3 pad: 1 FILL } }
layer { name: "r0" type: "ReLU" bottom: "c0" top: "c0" }
layer { name: "a17" type: "Convolution" bottom: "c0" top: "a17" convolution_param { num_output: 8 kernel_h: 1 kernel_w: 7 pad_h: 0 pad_w: 3 FILL } }
layer { name: "ra17" type: "ReLU" bottom: "a17" top: "a17" }
layer { name: "a71" type: "Convolution" bottom: "c0" top: "a71" convolution_param { num_output: 8 kernel_h: 7 kernel_w: 1 pad_h: 3 pad_w: 0 bias_term: false FILL } }
layer { name: "d2" type: "Convolution" bottom: "c0" top: "d2" convolution_param { num_output: 8 kernel_size: 3 pad: 2 dilation: 2 FILL } }
layer { name: "d4" type: "Convolution" bottom: "c0" top: "d4" convolution_param { num_output: 8 kernel_size: 3 pad: 4 dilation: 4 FILL } }
layer { name: "sum" type: "Eltwise" bottom: "a17" bottom: "a71" bottom: "d2" bottom: "d4" top: "sum" }
layer { name: "out" type: "Convolution" bottom: "sum" top: "out" convolution_param { num_output: 5 kernel_size: 3 pad: 3 dilation: 3 FILL } }
""".replace("FILL", FILL)


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, f16=True)


def rconv_tasks(e):
    return {t.layer.name: t for t in e.tasks if isinstance(t, E.OpTask) and t.rconv is not None}


def test_descriptors_over_halves(stub):
    e = stub(NET, rconv_f16=True)
    rt = rconv_tasks(e)
    assert sorted(rt) == ["a17", "a71", "d2", "d4", "out"] and all(t.ops == [] for t in rt.values())
    assert "ra17" not in [t.layer.name for t in e.tasks]                    # the in-place ReLU rides in a17's epilogue
    x = e.blobs["c0"]
    assert x.esize == 2 and x.cstride == 8
    for nm, (kh, kw, ph, pw, dil), relu in (("a17", (1, 7, 0, 3, 1), True), ("a71", (7, 1, 3, 0, 1), False), ("d2", (3, 3, 2, 2, 2), False),
                                            ("d4", (3, 3, 4, 4, 4), False)):
        d, y, pd = rt[nm].rconv, e.blobs[nm], e.params_dev[nm]
        assert y.esize == 2
        assert (d.x, d.Cin, d.x_cstride, d.N, d.H, d.W) == (x.ptr, 6, 8, 2, 12, 14)
        assert (d.y, d.Cout, d.y_coffset, d.y_cstride, d.OH, d.OW) == (y.buf.ptr, 8, y.coffset, y.cstride, 12, 14)
        assert (d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.dilation) == (kh, kw, ph, pw, 1, 1, dil)
        assert d.w == pd[0].ptr and d.bias == (pd[1].ptr if len(pd) > 1 else None)      # the parameter blob where it lies: no repacking
        assert d.flags == (L.CONV_RELU if relu else 0) and not d.y2
        seg = e.param_segs[(nm, 0)]
        assert seg.shape == (8, kh, kw, 8) and seg.esize == 2                            # [Cout][kh][kw][round8(Cin)] in halves
    d, y = rt["out"].rconv, e.blobs["out"]      # a net output: float32
    assert y.esize == 4 and e.blobs["sum"].esize == 2
    assert d.flags == L.CONV_OUT_F32 and (d.x, d.x_cstride, d.Cin, d.Cout, d.dilation) == (e.blobs["sum"].ptr, 8, 8, 5, 3)
    assert (d.y, d.y_cstride, d.y_coffset) == (y.buf.ptr, y.cstride, y.coffset)


def test_shared_plans_go_through_the_half_entry_points(stub):
    e = stub(NET, rconv_f16=True)
    rt = rconv_tasks(e)
    lv = dict(zip([t.layer.name for t in e.tasks], E.task_levels(e.tasks)))
    assert lv["a17"] == lv["a71"] == lv["d2"] == lv["d4"] == lv["c0"] + 1 and lv["out"] > lv["sum"] > lv["a17"]
    del e.fake.calls[:]
    e._emit_rconvs([rt[n] for n in ("a17", "a71", "d2", "d4")])
    assert e.fake.names().count("fcn_rconv2d_prepare_f16") == 2 and "fcn_rconv2d_prepare" not in e.fake.names()
    assert [(op.kind, op.name.split(" ")[0]) for op in e.ops] == [("dconv", "d2+d4"), ("rconv", "a17+a71")]      # square launches first
    assert e.ops[0].name.startswith("d2+d4 [d2,4 ") and e.ops[1].name.startswith("a17+a71 [1x7,7x1 ")
    op = e.ops[1]
    assert op.flops == 2 * (2.0 * 2 * 12 * 14 * 6 * 8 * 7)
    assert op.bytes == 2.0 * (2 * (2 * 6 * 168 + 2 * 8 * 168 + 8 * 6 * 7)) + 4.0 * (8 + 8)      # halves; the bias is float32
    for op in e.ops:
        op.run(None)
        assert e.fake.names()[-1] == "fcn_rconv2d_f16"
    e._emit_rconvs([rt["out"]])
    assert e.ops[2].kind == "dconv" and e.ops[2].bytes == 2.0 * (2 * 8 * 168 + 5 * 8 * 9) + 4.0 * (2 * 5 * 168 + 5)      # float32 result
    # the whole plan: one launch per kind and shared bottom
    e = stub(NET, rconv_f16=True)
    e.tuner = None
    del e.fake.calls[:]
    e._build_ops()
    assert [(op.kind, op.name.split(" ")[0]) for op in e.ops if op.kind in ("rconv", "dconv")] == [("dconv", "d2+d4"), ("rconv", "a17+a71"),
                                                                                                  ("dconv", "out")]
    assert e.fake.names().count("fcn_rconv2d_prepare_f16") == 3 and "fcn_rconv2d_prepare" not in e.fake.names()


def test_refusals_name_the_layer(stub):
    rect, dil = "kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 1", "kernel_size: 3 pad: 2 dilation: 2"
    # a float32 bottom: the layer sits on the image
    with pytest.raises(NotImplementedError, match=r"f16 engine: Convolution rect with dilation 2 reads the float32 blob data"):
        stub(one(dil, bottom="data"), rconv_f16=True)
    with pytest.raises(NotImplementedError, match=r"f16 engine: rectangular Convolution rect \(1x3 stride 1x1 pad 0x1\) reads the float32 blob data"):
        stub(one(rect, bottom="data"), rconv_f16=True)
    with pytest.raises(NotImplementedError, match=r"rectangular Convolution rect \(1x3 stride 1x1 pad 0x1\): group 2"):
        stub(one(rect + " group: 2").replace("num_output: 8", "num_output: 16"), rconv_f16=True)
    with pytest.raises(NotImplementedError, match=r"Convolution rect: group 2 together with dilation 2"):
        stub(one(dil + " group: 2").replace("num_output: 8", "num_output: 16"), rconv_f16=True)
    # a window that does not start on 16 bytes of halves: the second bottom of a Concat behind 4 channels
    e = stub(one(dil), rconv_f16=True)
    by = {l.name: l for l in e.spec.layers}
    xb = e.blobs["c0"]
    li = e.spec.layers.index(by["rect"])
    assert e._rconv_task(li, by["rect"], set()).rconv.x == xb.ptr
    xb.coffset = 4      # (a float32 engine takes a window at 4 channels: 16 bytes of floats)
    with pytest.raises(NotImplementedError, match=r"dilated Convolution rect: input view is not 16-byte aligned"):
        e._rconv_task(li, by["rect"], set())


def test_a_bare_netspec_refuses_as_before(stub):
    with pytest.raises(NotImplementedError) as ei:
        stub(one("kernel_h: 1 kernel_w: 3 pad_h: 0 pad_w: 1"))
    assert str(ei.value) == "f16 engine: rectangular Convolution rect (1x3 stride 1x1 pad 0x1) has no half-float kernel"
    with pytest.raises(NotImplementedError) as ei:
        stub(one("kernel_size: 3 pad: 2 dilation: 2"))
    assert str(ei.value) == "f16 engine: Convolution rect with dilation 2 has no half-float kernel"
    with pytest.raises(NotImplementedError) as ei:
        stub(NET)
    assert str(ei.value) == "f16 engine: rectangular Convolution a17 (1x7 stride 1x1 pad 0x3) has no half-float kernel"
    assert NetSpec(proto.parse_text(NET)).rconv_f16 is False and NetSpec(proto.parse_text(NET), rconv_f16=True).rconv_f16 is True


def test_the_float32_plan_does_not_depend_on_the_keyword(stub):
    for text in (NET, models.deeplab_aspp("DEPLOY", batch=1, num_classes=5, width_div=8, fc_div=8, size=65)):
        a, b = stub(text, f16=False), stub(text, f16=False, rconv_f16=True)
        sa, sb = plan_signature(a), plan_signature(b)
        assert sa == sb and any(r.get("rconv") for r in sa)
        for e in (a, b):
            e.tuner = None
            del e.fake.calls[:]
            e._build_ops()
            assert "fcn_rconv2d_prepare_f16" not in e.fake.names() and e.fake.names().count("fcn_rconv2d_prepare") >= 1
        assert [(op.kind, op.name, op.flops, op.bytes) for op in a.ops] == [(op.kind, op.name, op.flops, op.bytes) for op in b.ops]


def writers_nets():
    lf = dict(batch=1, num_classes=5, width_div=8, fc_div=8, size=65)
    return [("largefov", models.deeplab_largefov("DEPLOY", **lf), 4, "conv5_1"),
            ("largefov interp argmax", models.deeplab_largefov("DEPLOY", interp=True, argmax=True, **lf), 4, "conv5_1"),
            ("aspp interp", models.deeplab_aspp("DEPLOY", interp=True, **lf), 7, "conv5_1"),
            ("aspp interp argmax", models.deeplab_aspp("DEPLOY", interp=True, argmax=True, **lf), 7, "conv5_1"),
            ("inception_v3 /4", models.inception_v3("DEPLOY", batch=1, classes=10, width_div=4), 34, "mixed_17a/7x7_1x7")]


@pytest.mark.parametrize("name,text,problems,first", writers_nets(), ids=[n[0] for n in writers_nets()])
def test_the_writers_nets_plan_completely(stub, name, text, problems, first):
    with pytest.raises(NotImplementedError, match="f16 engine: .*%s.* has no half-float kernel" % first):
        stub(text, depthwise=True, ip_gemm=True)
    e = stub(text, depthwise=True, ip_gemm=True, rconv_f16=True)
    rt = rconv_tasks(e)
    assert len(rt) == problems
    for nm, t in rt.items():      # the aligned form on every real layer
        d, l = t.rconv, t.layer
        xb, yb = e.blobs[l.bottoms[0]], e.blobs[l.tops[0]]
        assert xb.esize == 2 and yb.esize == 2 and not d.flags & L.CONV_OUT_F32, nm
        assert xb.cstride % 8 == 0 and xb.coffset % 8 == 0 and yb.coffset % 8 == 0, nm
        assert e.param_segs[(nm, 0)].esize == 2 and e.param_segs[(nm, 0)].shape[-1] == (d.Cin + 7) // 8 * 8, nm
    e.tuner = None
    del e.fake.calls[:]
    e._build_ops()
    assert e.fake.names().count("fcn_rconv2d_prepare_f16") >= 1 and "fcn_rconv2d_prepare" not in e.fake.names()
