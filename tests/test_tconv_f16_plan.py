"""The group-1 Deconvolution and the converting Crop as the half-float forward planner lays them out - without a GPU.

The half-float stub engine of tests/plan_stub.py over a NetSpec built with tconv_f16=True, on the published FCN-32s / 16s / 8s nets at 5
classes, 64 x 48 and an eighth of the widths: without the keyword each is refused by the name of its first group-1 Deconvolution in
the words it always was; with it each plans completely - tconv_pack + tconv through the half entry points, descriptors over halves, the
bank segment in halves, `score` float32 through the converting crop or half in front of ArgMax.  The float32 plan of the same nets does
not depend on the keyword, and a Crop from a float32 bottom into a half top is still refused."""
from collections import namedtuple

import numpy as np
import pytest

from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd import storage as S
from fcn_object_detector_amd.netspec import NetSpec
from plan_stub import engine_factory
from test_rect_plan import FILL, plan_signature

KW = dict(num_classes=5, shape=(1, 3, 64, 48), width_div=8, fillers=True)
# variant -> (writer, its group-1 Deconvolutions in layer order as (name, k, s), the Crop that writes `score`)
NETS = {32: (models.voc_fcn32s, [("upscore", 64, 32)]),
        16: (models.voc_fcn16s, [("upscore2", 4, 2), ("upscore16", 32, 16)]),
        8: (models.voc_fcn8s, [("upscore2", 4, 2), ("upscore_pool4", 4, 2), ("upscore8", 16, 8)])}
PUBLIC = dict(depthwise=True, ip_gemm=True, rconv_f16=True)
View = namedtuple("View", "esize")      # what storage.param_layout reads of a bottom's view in these nets


@pytest.fixture
def stub(monkeypatch):
    return engine_factory(monkeypatch, f16=True)


def built(e):
    e.tuner = None
    del e.fake.calls[:]
    e._build_ops()
    return e


@pytest.mark.parametrize("argmax", [False, True], ids=["score", "argmax"])
@pytest.mark.parametrize("variant", [32, 16, 8])
def test_without_the_keyword_the_first_deconvolution_is_refused_as_before(stub, variant, argmax):
    writer, deconvs = NETS[variant]
    with pytest.raises(NotImplementedError) as ei:
        stub(writer("TEST", argmax=argmax, **KW), **PUBLIC)
    assert str(ei.value) == "f16 engine: layer type Deconvolution with group 1 (%s) has no half-float kernel" % deconvs[0][0]
    assert NetSpec(proto.parse_text(writer("TEST", **KW))).tconv_f16 is False
    assert NetSpec(proto.parse_text(writer("TEST", **KW)), tconv_f16=True).tconv_f16 is True


@pytest.mark.parametrize("argmax", [False, True], ids=["score", "argmax"])
@pytest.mark.parametrize("variant", [32, 16, 8])
def test_the_published_nets_plan_completely(stub, variant, argmax):
    writer, deconvs = NETS[variant]
    e = built(stub(writer("TEST", argmax=argmax, **KW), tconv_f16=True, **PUBLIC))
    by = {l.name: l for l in e.spec.layers}
    ops = [(op.kind, op.name) for op in e.ops]
    # every group-1 Deconvolution: a bank of halves, re-packed and launched through the half entry points
    assert e.fake.names().count("fcn_tconv2d_prepare_f16") == len(deconvs) and "fcn_tconv2d_prepare" not in e.fake.names()
    descs = [k for k in e._keep if isinstance(k, L.TConvDesc)][-len(deconvs):]      # (of this _build_ops: the fixture has planned once before)
    for (name, k, s), d in zip(deconvs, descs):
        l = by[name]
        xb, yb = e.blobs[l.bottoms[0]], e.blobs[l.tops[0]]
        seg = e.param_segs[(name, 0)]
        assert seg.kind == S.DECONV and seg.esize == 2 and seg.shape == (5, k, k, 8) and seg.nbytes == 5 * k * k * 8 * 2
        assert xb.esize == 2 and yb.esize == 2 and xb.cstride % 8 == 0 and xb.coffset % 8 == 0
        assert (d.a, d.Ca, d.a_cstride, d.N, d.H, d.W) == (xb.ptr, 5, xb.cstride, 1) + tuple(xb.shape[2:])
        assert (d.b, d.Cb, d.b_cstride, d.b_coffset, d.OH, d.OW) == (yb.buf.ptr, 5, yb.cstride, yb.coffset) + tuple(yb.shape[2:])
        assert (d.kh, d.kw, d.stride, d.pad, d.flags, d.bias) == (k, k, s, 0, 0, None) and not d.y2
        assert d.OH == s * (d.H - 1) + k
        i = ops.index(("tconv_pack", name))
        assert ops[i + 1] == ("tconv", name)
        del e.fake.calls[:]
        e.ops[i].run(None)
        e.ops[i + 1].run(None)
        assert e.fake.names() == ["fcn_tconv_bank_pack_f16", "fcn_tconv2d_f16"]
        assert e.ops[i + 1].bytes == 2.0 * xb.pixels * 5 + 2.0 * yb.pixels * 5
    # the tail: the last transposed convolution, the crop to `score`, the label map
    kinds = [k for k, _ in ops]
    last = ops.index(("tconv", deconvs[-1][0]))
    assert kinds[last + 1:] == ["crop"] + (["argmax"] if argmax else [])
    score, up = e.blobs["score"], e.blobs[deconvs[-1][0]]
    assert up.esize == 2 and score.esize == (2 if argmax else 4) and score.shape == (1, 5, 64, 48)
    del e.fake.calls[:]
    e.ops[last + 1].run(None)
    assert e.fake.names() == ["fcn_crop_fwd_f16" if argmax else "fcn_crop_fwd_f16_f32"]
    assert e.ops[last + 1].bytes == float(2 + score.esize) * 64 * 48 * 5
    if argmax:
        assert e.blobs["argmax"].esize == 4 and e.outputs == ["argmax"]
    # the skip crops copy between half blobs
    for l in e.spec.layers:
        if l.type == "Crop" and l.tops[0] != "score":
            assert e.blobs[l.bottoms[0]].esize == e.blobs[l.tops[0]].esize == 2, l.name
    assert kinds.count("crop") == {32: 1, 16: 2, 8: 3}[variant] and kinds.count("eltwise") == {32: 0, 16: 1, 8: 2}[variant]


def test_the_bank_of_halves_packs_and_reads_back_as_float32(stub):
    e = stub(models.voc_fcn16s("TEST", **KW), tconv_f16=True, **PUBLIC)
    seg = e.param_segs[("upscore2", 0)]
    w = np.random.default_rng(0).standard_normal(seg.host_shape).astype(np.float32)
    dev = S.pack(seg, w)
    assert dev.dtype == np.float16 and dev.shape == (5, 4, 4, 8) and not dev[..., 5:].any()
    assert np.array_equal(dev[..., :5], w.astype(np.float16).transpose(0, 2, 3, 1))
    back = S.unpack(seg, dev.reshape(-1).view(np.uint8))
    assert back.dtype == np.float32 and back.shape == seg.host_shape and np.array_equal(back, w.astype(np.float16).astype(np.float32))


def test_the_float32_plan_does_not_depend_on_the_keyword(stub):
    for variant in (32, 16, 8):
        text = NETS[variant][0]("TEST", **KW)
        a, b = stub(text, f16=False, **PUBLIC), stub(text, f16=False, tconv_f16=True, **PUBLIC)
        assert plan_signature(a) == plan_signature(b)
        assert [(s.kind, s.shape, s.esize, s.offset) for s in a.param_segs.values()] == [(s.kind, s.shape, s.esize, s.offset) for s in b.param_segs.values()]
        for e in (a, b):
            built(e)
            assert "fcn_tconv2d_prepare_f16" not in e.fake.names() and e.fake.names().count("fcn_tconv2d_prepare") == len(NETS[variant][1])
        assert [(op.kind, op.name, op.flops, op.bytes) for op in a.ops] == [(op.kind, op.name, op.flops, op.bytes) for op in b.ops]
        for op in a.ops:
            if op.kind in ("tconv_pack", "tconv", "crop"):
                del a.fake.calls[:]
                op.run(None)
                assert a.fake.names()[0] in ("fcn_tconv_bank_pack_f32", "fcn_tconv2d_f32", "fcn_crop_fwd_f32")


TINY = """
input: "data" input_shape { dim: 1 dim: 3 dim: 8 dim: 8 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 5 kernel_size: 3 pad: 1 FILL } }
layer { name: "up" type: "Deconvolution" bottom: "BOTTOM" top: "up" convolution_param { num_output: 5 kernel_size: 4 stride: 2 FILL } }
layer { name: "score" type: "Crop" bottom: "up" bottom: "data" top: "score" crop_param { axis: 2 offset: 5 } }
""".replace("FILL", FILL)


def test_refusals_name_the_layer(stub):
    e = built(stub(TINY.replace("BOTTOM", "c0"), tconv_f16=True))
    assert [op.kind for op in e.ops][-3:] == ["tconv_pack", "tconv", "crop"] and e.blobs["score"].esize == 4
    d = [k for k in e._keep if isinstance(k, L.TConvDesc)][-1]
    assert d.bias == e.params_dev["up"][1].ptr and e.param_segs[("up", 1)].esize == 4      # the bias stays float32
    # a float32 bottom: the layer sits on the image
    with pytest.raises(NotImplementedError, match=r"f16 engine: Deconvolution up reads the float32 blob data"):
        stub(TINY.replace("BOTTOM", "data").replace("dim: 3 dim: 8", "dim: 5 dim: 8"), tconv_f16=True)
    # a window that does not start on 16 bytes of halves
    e = stub(TINY.replace("BOTTOM", "c0"), tconv_f16=True)
    e.blobs["c0"].coffset = 4      # (a float32 engine takes a window at 4 channels: 16 bytes of floats)
    by = {l.name: l for l in e.spec.layers}
    with pytest.raises(NotImplementedError, match=r"Deconvolution up: input view is not 16-byte aligned"):
        e._fwd_deconvolution(by["up"], ["c0"])
    # half-float training
    with pytest.raises(NotImplementedError, match=r"f16 engine: Deconvolution up with group 1 in a TRAIN net \(half-float training\)"):
        spec = NetSpec(proto.parse_text(TINY.replace("BOTTOM", "c0")), "TRAIN", tconv_f16=True)
        spec.infer()
        S.param_layout(spec, {name: View(2) for name in ("data", "c0", "up")}, True)
    # without the keyword: today's words
    with pytest.raises(NotImplementedError) as ei:
        stub(TINY.replace("BOTTOM", "c0"))
    assert str(ei.value) == "f16 engine: layer type Deconvolution with group 1 (up) has no half-float kernel"


MIXED = """
input: "data" input_shape { dim: 1 dim: 8 dim: 12 dim: 12 }
input: "like" input_shape { dim: 1 dim: 8 dim: 8 dim: 8 }
layer { name: "cut" type: "Crop" bottom: "data" bottom: "like" top: "cut" crop_param { axis: 2 offset: 2 } }
layer { name: "c0" type: "Convolution" bottom: "cut" top: "c0" convolution_param { num_output: 8 kernel_size: 3 pad: 1 FILL } }
layer { name: "c1" type: "Convolution" bottom: "c0" top: "c1" convolution_param { num_output: 8 kernel_size: 3 pad: 1 FILL } }
""".replace("FILL", FILL)


def test_the_mixed_direction_crop_is_still_refused(stub):
    """A float32 bottom (a net input) into a half top."""
    with pytest.raises(NotImplementedError, match=r"f16 engine: Crop cut copies between half and float32 blobs"):
        stub(MIXED, tconv_f16=True)
    stub(MIXED, f16=False, tconv_f16=True)


def test_other_producers_of_a_float32_output_stay_refused(stub):
    net = TINY.replace("BOTTOM", "c0") + 'layer { name: "p" type: "Pooling" bottom: "up" top: "p" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }\n'
    with pytest.raises(NotImplementedError, match=r"f16 engine: float32 blob p is produced by \['Pooling'\]"):
        stub(net, tconv_f16=True)
