"""Depthwise convolution in the net description and the parameter layout - without a GPU: both spellings (type DepthwiseConvolution;
type Convolution with group == channels == num_output under NetSpec(depthwise=True)), their shapes and blobs, every malformed form by
layer name, the DEPTHWISE segment of the flat parameter buffer and its pack / unpack round trip, and the MobileNet writers."""
import numpy as np
import pytest

from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd import storage as S
from fcn_object_detector_amd.netspec import NetSpec, fill_params

HEAD = 'input: "data" input_shape { dim: 2 dim: 6 dim: 9 dim: 11 }\n'


def dw_layer(body, type_="DepthwiseConvolution", name="dw"):
    return HEAD + 'layer { name: "%s" type: "%s" bottom: "data" top: "%s" convolution_param { %s } }\n' % (name, type_, name, body)


def spec_of(text, **kw):
    s = NetSpec(proto.parse_text(text), "TEST", **kw)
    s.infer()
    return s


class View:
    """What storage.param_layout asks of a blob view."""
    def __init__(self, esize):
        self.esize = esize


@pytest.mark.parametrize("body,shape,blobs", [
    ("num_output: 6 kernel_size: 3 pad: 1", (2, 6, 9, 11), [(6, 1, 3, 3), (6,)]),
    ("num_output: 6 group: 6 kernel_size: 3 pad: 1 stride: 2 bias_term: false", (2, 6, 5, 6), [(6, 1, 3, 3)]),
    ("num_output: 6 group: 6 kernel_h: 3 kernel_w: 5 pad_h: 0 pad_w: 2 stride_h: 2 stride_w: 1", (2, 6, 4, 11), [(6, 1, 3, 5), (6,)]),
    ("num_output: 6 kernel_size: 3 pad: 2 dilation: 2 engine: CAFFE", (2, 6, 9, 11), [(6, 1, 3, 3), (6,)]),
    ("num_output: 6 kernel_size: 1 stride: 2", (2, 6, 5, 6), [(6, 1, 1, 1), (6,)])])
def test_the_layer_type_gives_caffes_shapes_and_blobs(body, shape, blobs):
    for kw in ({}, {"depthwise": True}):      # the type needs no keyword
        s = spec_of(dw_layer(body), **kw)
        assert s.blob_shapes["dw"] == shape and s.param_shapes["dw"] == blobs
        assert s.is_depthwise(s.layers[0])


def test_the_keyword_makes_the_published_spelling_the_same_thing():
    body = "num_output: 6 group: 6 kernel_size: 3 pad: 1 stride: 2 bias_term: false engine: CAFFE"
    bare, keyed = spec_of(dw_layer(body, "Convolution")), spec_of(dw_layer(body, "Convolution"), depthwise=True)
    typed = spec_of(dw_layer(body))
    assert bare.blob_shapes == keyed.blob_shapes == typed.blob_shapes and bare.param_shapes == keyed.param_shapes == typed.param_shapes
    assert keyed.is_depthwise(keyed.layers[0]) and typed.is_depthwise(typed.layers[0]) and not bare.is_depthwise(bare.layers[0])
    # group 1, a group that is not the channel count, one channel: ordinary convolutions under the keyword too
    for other in ("num_output: 6 kernel_size: 3", "num_output: 6 group: 3 kernel_size: 3", "num_output: 6 group: 2 kernel_size: 3"):
        s = spec_of(dw_layer(other, "Convolution"), depthwise=True)
        assert not s.is_depthwise(s.layers[0])
    one = spec_of(HEAD.replace("dim: 6", "dim: 1") + 'layer { name: "c" type: "Convolution" bottom: "data" top: "c" convolution_param { num_output: 1 kernel_size: 3 } }',
                  depthwise=True)
    assert not one.is_depthwise(one.layers[0])
    assert NetSpec.from_file.__defaults__ == ("TEST", False)


def test_a_bare_netspec_keeps_the_refusal_and_names_the_keyword():
    s = spec_of(dw_layer("num_output: 6 group: 6 kernel_size: 3 pad: 1", "Convolution"))
    with pytest.raises(NotImplementedError, match=r"grouped Convolution dw: group 6 .*depthwise convolution has no kernel here.*depthwise=True"):
        S.param_layout(s, {"data": View(4)}, False)


@pytest.mark.parametrize("body,err,match", [
    ("num_output: 12 kernel_size: 3", NotImplementedError, r"layer dw: .*channel multiplier of 2"),
    ("num_output: 12 group: 6 kernel_size: 3", NotImplementedError, r"layer dw: .*channel multiplier of 2"),
    ("num_output: 6 group: 3 kernel_size: 3", ValueError, r"layer dw: DepthwiseConvolution over 6 channels with group 3, num_output 6"),
    ("num_output: 6 group: 1 kernel_size: 3", ValueError, r"layer dw: .*group 1"),
    ("num_output: 4 kernel_size: 3", ValueError, r"layer dw: .*num_output 4"),
    ("num_output: 9 group: 6 kernel_size: 3", ValueError, r"layer dw: .*num_output 9"),
    ("kernel_size: 3", ValueError, r"layer dw: DepthwiseConvolution without num_output"),
    ("num_output: 6", ValueError, r"layer dw without kernel_size"),
    ("num_output: 6 kernel_size: 3 kernel_h: 3 kernel_w: 3", ValueError, r"layer dw: both kernel_size and kernel_h"),
    ("num_output: 6 kernel_size: 3 stride: 0", ValueError, r"layer dw: stride 0x0 is below 1"),
    ("num_output: 6 kernel_size: 3 pad_h: 1", ValueError, r"layer dw: pad_h without pad_w"),
    ("num_output: 6 kernel_size: 3 dilation: 2 dilation: 3", NotImplementedError, r"layer dw: dilation \[2, 3\]"),
    ("num_output: 6 kernel_size: 7 dilation: 2", ValueError, r"layer dw: the 7x7 window with dilation 2 exceeds the padded 9x11 bottom")])
def test_malformed_layers_are_refused_by_name(body, err, match):
    with pytest.raises(err, match=match):
        spec_of(dw_layer(body))


def test_two_bottoms_and_the_multiplier_under_the_keyword_are_refused_by_name():
    two = HEAD + 'layer { name: "dw" type: "DepthwiseConvolution" bottom: "data" bottom: "data" top: "dw" convolution_param { num_output: 6 kernel_size: 3 } }'
    with pytest.raises(ValueError, match="layer dw: DepthwiseConvolution takes one 4-d bottom"):
        spec_of(two)
    with pytest.raises(NotImplementedError, match=r"layer dw: depthwise Convolution over 6 channels with num_output 12 \(a channel multiplier of 2"):
        spec_of(dw_layer("num_output: 12 group: 6 kernel_size: 3", "Convolution"), depthwise=True)


@pytest.mark.parametrize("type_,kw", [("DepthwiseConvolution", {}), ("Convolution", {"depthwise": True})])
def test_the_depthwise_segment_and_its_round_trip(type_, kw):
    text = dw_layer("num_output: 6 group: 6 kernel_h: 3 kernel_w: 5 pad_h: 1 pad_w: 2", type_) + \
        'layer { name: "pw" type: "Convolution" bottom: "dw" top: "pw" convolution_param { num_output: 5 kernel_size: 1 } }\n'
    s = spec_of(text, **kw)
    for esize, cpad in ((4, 8), (2, 8)):
        views = {"data": View(esize), "dw": View(esize)}
        segs, total = S.param_layout(s, views, esize == 2)
        w, b, pw = segs[0], segs[1], segs[2]
        assert (w.layer, w.kind, w.shape, w.host_shape, w.esize, w.offset) == ("dw", S.DEPTHWISE, (3, 5, cpad), (6, 1, 3, 5), 4, 0)      # always float32
        assert (b.kind, b.shape, b.offset) == (S.PLAIN, (6,), 3 * 5 * cpad)
        assert (pw.layer, pw.kind, pw.shape, pw.esize, pw.offset) == ("pw", S.CONV, (5, 1, 1, cpad), esize, 3 * 5 * cpad + 8)      # everything else as before
        blob = np.random.default_rng(1).standard_normal((6, 1, 3, 5)).astype(np.float32)
        packed = S.pack(w, blob)
        assert packed.shape == (3, 5, cpad) and packed.dtype == np.float32
        assert np.array_equal(packed[1, 4, :6], blob[:, 0, 1, 4]) and not packed[..., 6:].any()      # tap-major, channel-contiguous, pad channels zero
        back = S.unpack(w, packed.view(np.uint8).reshape(-1))
        assert back.shape == (6, 1, 3, 5) and back.dtype == np.float32 and np.array_equal(back, blob)
    assert S.param_layout(s, {"data": View(4), "dw": View(4)}, False)[0][0].shape == (3, 5, 8)
    c4 = spec_of(text.replace("dim: 6", "dim: 4").replace("num_output: 6 group: 6", "num_output: 4 group: 4"), **kw)
    assert S.param_layout(c4, {"data": View(4), "dw": View(4)}, False)[0][0].shape == (3, 5, 4)


def _net(text, phase):
    s = NetSpec(proto.parse_text(text), phase, depthwise=True)
    s.infer()
    return s


def test_mobilenet_v1_at_full_width():
    for phase, net_phase in (("DEPLOY", "TEST"), ("TRAIN", "TRAIN"), ("TEST", "TEST")):
        s = _net(models.mobilenet_v1(phase), net_phase)
        dws = [l for l in s.layers if s.is_depthwise(l)]
        assert len(dws) == 13 and [l.name for l in dws][:2] == ["conv2_1/dw", "conv2_2/dw"] and dws[-1].name == "conv6/dw"
        assert all(l.type == "Convolution" and str(l.sub("convolution_param").get("engine")) == "CAFFE" for l in dws)      # as published
        assert [int(l.sub("convolution_param").get("stride")) for l in dws] == [1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1]
        assert [s.blob_shapes[l.tops[0]][1] for l in dws] == [32, 64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024]
        assert s.blob_shapes["conv6/sep"] == (1, 1024, 7, 7) and s.blob_shapes["pool6"] == (1, 1024, 1, 1) and s.blob_shapes["fc7"] == (1, 1000, 1, 1)
        assert s.param_shapes["conv2_1/dw"] == [(32, 1, 3, 3)] and s.param_shapes["conv2_1/sep"] == [(64, 32, 1, 1)]      # bias-free
        assert s.param_shapes["fc7"] == [(1000, 1024, 1, 1), (1000,)]
        convs = [l for l in s.layers if l.type == "Convolution"]
        assert len(convs) == 28 and sum(l.type == "BatchNorm" for l in s.layers) == sum(l.type == "Scale" for l in s.layers) == 27
        assert sum(l.type == "ReLU" for l in s.layers) == 27
        assert s.output_blobs() == {"DEPLOY": ["prob"], "TRAIN": ["loss"], "TEST": ["accuracy", "loss"]}[phase]
    assert "_filler" not in models.mobilenet_v1("DEPLOY", fillers=False)
    with pytest.raises(ValueError):
        models.mobilenet_v1("FINETUNE")


def test_mobilenet_v2_at_full_width():
    s = _net(models.mobilenet_v2("TRAIN", batch=2), "TRAIN")
    dws = [l for l in s.layers if s.is_depthwise(l)]
    assert len(dws) == 17 and sum(l.type == "Eltwise" for l in s.layers) == 10
    assert [l.name for l in dws][:3] == ["conv2_1/dwise", "conv3_1/dwise", "conv3_2/dwise"]
    assert "conv2_1/expand" not in s.param_shapes and s.param_shapes["conv3_1/expand"] == [(96, 16, 1, 1)]      # t = 1: no expansion
    assert s.param_shapes["conv3_1/dwise"] == [(96, 1, 3, 3)] and s.param_shapes["conv3_1/linear"] == [(24, 96, 1, 1)]
    assert [s.blob_shapes[n] for n in ("conv2_1/linear", "conv3_1/linear", "block_3_2", "block_4_3", "block_5_4", "block_6_3", "block_7_3", "conv8_1/linear",
                                       "conv9", "pool6", "fc7")] == \
        [(2, 16, 112, 112), (2, 24, 56, 56), (2, 24, 56, 56), (2, 32, 28, 28), (2, 64, 14, 14), (2, 96, 14, 14), (2, 160, 7, 7), (2, 320, 7, 7),
         (2, 1280, 7, 7), (2, 1280, 1, 1), (2, 1000, 1, 1)]
    # a linear bottleneck has no ReLU, and a block's sum reads the block's input
    by = {l.name: l for l in s.layers}
    assert not any(l.type == "ReLU" and l.bottoms == ["conv3_1/linear"] for l in s.layers)
    assert by["block_3_2"].bottoms == ["conv3_1/linear", "conv3_2/linear"] and by["block_4_3"].bottoms == ["block_4_2", "conv4_3/linear"]
    assert [int(l.sub("convolution_param").get("stride")) for l in dws] == [1, 2, 1, 2, 1, 1, 2, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1]
    assert _net(models.mobilenet_v2("DEPLOY"), "TEST").output_blobs() == ["prob"]


def test_the_writers_at_an_eighth_of_the_width():
    s = _net(models.mobilenet_v1("TRAIN", batch=4, classes=6, width_div=8, size=128), "TRAIN")
    dws = [l for l in s.layers if s.is_depthwise(l)]
    assert len(dws) == 13 and [s.blob_shapes[l.tops[0]][1] for l in dws] == [4, 8, 16, 16, 32, 32, 64, 64, 64, 64, 64, 64, 128]
    assert s.blob_shapes["conv6/sep"] == (4, 128, 4, 4) and s.blob_shapes["fc7"] == (4, 6, 1, 1) and s.blob_shapes["label"] == (4, 1, 1, 1)
    params = fill_params(s, seed=3)
    assert params["conv2_1/dw"][0].shape == (4, 1, 3, 3) and abs(float(params["conv5_3/dw"][0].std()) - (2.0 / 9) ** 0.5) < 0.05
    s2 = _net(models.mobilenet_v2("DEPLOY", batch=1, classes=6, width_div=8, size=64), "TEST")
    assert len([l for l in s2.layers if s2.is_depthwise(l)]) == 17 and sum(l.type == "Eltwise" for l in s2.layers) == 10
    assert s2.blob_shapes["conv9"] == (1, 160, 2, 2) and s2.blob_shapes["prob"] == (1, 6, 1, 1)
    # every segment of the flat buffer: the depthwise banks are DEPTHWISE, the rest as before
    views = {n: View(4) for n in s.blob_shapes}
    segs, _ = S.param_layout(s, views, False)
    kinds = {(g.layer, g.index): g.kind for g in segs}
    assert all(kinds[(l.name, 0)] == S.DEPTHWISE for l in dws) and kinds[("conv2_1/sep", 0)] == S.CONV and kinds[("fc7", 1)] == S.PLAIN
