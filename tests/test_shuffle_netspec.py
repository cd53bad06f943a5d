"""ShuffleChannel and the ConvolutionDepthwise spelling in the NetSpec, and the two ShuffleNet writers of models.py (no GPU).

Shapes on 4-d and 2-d blobs; a bare and a public NetSpec both take the layer (no keyword: FEATURES is unchanged); every refusal by layer
name and exception type; `type: "ConvolutionDepthwise"` is read as DepthwiseConvolution where the Layer is made, and refuses and infers
exactly as that type does; models.shufflenet_v1 / shufflenet_v2: layer counts, stage shapes in the three phases, the shortcut pooling of
a stride-2 unit on even and odd edges, the refused widths and groups with their channel counts, both depthwise_type spellings."""
import pytest

from fcn_object_detector_amd import models, netspec, proto
from fcn_object_detector_amd.netspec import Layer, NetSpec

DATA4 = 'layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 2 dim: 12 dim: 5 dim: 7 } } }\n'
DATA2 = 'layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 3 dim: 12 } } }\n'
SHUF = 'layer { name: "sh" type: "ShuffleChannel" bottom: "data" top: "y" %s }\n'


def spec_of(text, phase="TEST", public=False):
    msg = proto.parse_text(text)
    s = NetSpec.public(msg, phase) if public else NetSpec(msg, phase)
    s.infer()
    return s


@pytest.mark.parametrize("public", [False, True], ids=["bare", "public"])
@pytest.mark.parametrize("data,shape", [(DATA4, (2, 12, 5, 7)), (DATA2, (3, 12))], ids=["4-d", "2-d"])
def test_the_top_has_the_bottoms_shape_in_every_netspec(data, shape, public):
    for body in ("shuffle_channel_param { group: 3 }", "shuffle_channel_param { group: 12 }", ""):      # (the default group is 1)
        s = spec_of(data + SHUF % body, public=public)
        assert s.blob_shapes["y"] == shape and "sh" not in s.param_shapes and s.param_layers() == []
    l = s.layers[-1]
    assert netspec.shuffle_group(l, [shape]) == 1
    assert netspec.shuffle_group(Layer(proto.parse_text(SHUF % "shuffle_channel_param { group: 4 }").getall("layer")[0]), [shape]) == 4


def test_no_keyword_was_added():
    assert netspec.FEATURES == ("depthwise", "ip_gemm", "rconv_f16", "tconv_f16", "scale_gate", "activations")
    assert netspec.SHUFFLE_TYPES == ("ShuffleChannel",)
    assert not set(netspec.SHUFFLE_TYPES) & (set(netspec.NEURON_TYPES) | set(netspec.ACT_TYPES))


REFUSALS = [
    ("group 0", DATA4 + SHUF % "shuffle_channel_param { group: 0 }", ValueError, "layer sh: ShuffleChannel with group 0 over 12 channels"),
    ("a negative group", DATA4 + SHUF % "shuffle_channel_param { group: -2 }", ValueError, "layer sh: ShuffleChannel with group -2"),
    ("a group that does not divide", DATA4 + SHUF % "shuffle_channel_param { group: 5 }", ValueError, "layer sh: ShuffleChannel with group 5 over 12"),
    ("a second bottom", DATA4 + (SHUF % "").replace('top: "y"', 'bottom: "data" top: "y"'), ValueError, "layer sh: ShuffleChannel takes one bottom and has one top, got 2 and 1"),
    ("a second top", DATA4 + (SHUF % "").replace('top: "y"', 'top: "y" top: "z"'), ValueError, "layer sh: ShuffleChannel takes one bottom and has one top, got 1 and 2"),
    ("in place", DATA4 + (SHUF % "shuffle_channel_param { group: 3 }").replace('top: "y"', 'top: "data"'), ValueError, "layer sh: ShuffleChannel does not allow in-place"),
    ("a 3-d blob", 'layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 2 dim: 12 dim: 5 } } }\n' + SHUF % "", ValueError,
     "layer sh: ShuffleChannel takes one 4-d or 2-d bottom"),
]


@pytest.mark.parametrize("name,text,exc,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
@pytest.mark.parametrize("public", [False, True], ids=["bare", "public"])
def test_refusals_by_layer_name(name, text, exc, msg, public):
    with pytest.raises(exc, match=msg):
        spec_of(text, public=public)


def test_exp_log_and_threshold_keep_the_generic_refusal():
    for t in ("Exp", "Log", "Threshold", "ShuffleChannels"):
        with pytest.raises(NotImplementedError, match=r"layer type '%s' \(layer sh\)" % t):
            spec_of(DATA4 + (SHUF % "").replace("ShuffleChannel", t))


DW = ('layer { name: "dw" type: "%s" bottom: "data" top: "dw" convolution_param { num_output: %d kernel_size: 3 pad: 1 stride: 2 bias_term: false %s } }\n')


def test_convolution_depthwise_is_read_as_depthwise_convolution():
    a = spec_of(DATA4 + DW % ("ConvolutionDepthwise", 12, ""))
    b = spec_of(DATA4 + DW % ("DepthwiseConvolution", 12, ""))
    assert a.layers[-1].type == b.layers[-1].type == "DepthwiseConvolution" and a.is_depthwise(a.layers[-1])
    assert a.blob_shapes == b.blob_shapes and a.blob_shapes["dw"] == (2, 12, 3, 4) and a.param_shapes == b.param_shapes == {"dw": [(12, 1, 3, 3)]}
    assert spec_of(DATA4 + DW % ("ConvolutionDepthwise", 12, "group: 12")).blob_shapes == b.blob_shapes
    for num_output, extra, exc in ((24, "", NotImplementedError), (8, "", ValueError), (12, "group: 6", ValueError)):
        msgs = []
        for t in ("ConvolutionDepthwise", "DepthwiseConvolution"):
            with pytest.raises(exc) as info:
                spec_of(DATA4 + DW % (t, num_output, extra))
            msgs.append(str(info.value))
        assert msgs[0] == msgs[1] and "layer dw: DepthwiseConvolution" in msgs[0]
    assert Layer(proto.parse_text(DW % ("Convolution", 12, "group: 12")).getall("layer")[0]).type == "Convolution"      # nothing else is renamed


# ---------------------------------------------------------------------------------------------------------------- the writers
SMALL_V1 = dict(width_div=5, size=64, batch=2, classes=10)
SMALL_V2 = dict(width_div=3, size=64, batch=2, classes=10)


def infer(text, phase):
    s = NetSpec.public(proto.parse_text(text), "TEST" if phase == "DEPLOY" else phase)
    s.infer()
    return s


def count(s, t):
    return sum(1 for l in s.layers if l.type == t)


@pytest.mark.parametrize("phase,extra", [("DEPLOY", 1), ("TRAIN", 2), ("TEST", 3)])
@pytest.mark.parametrize("dwt", models.DEPTHWISE_TYPES)
def test_shufflenet_v1_layers_and_stage_shapes(phase, extra, dwt):
    s = infer(models.shufflenet_v1(phase, depthwise_type=dwt), phase)
    # per unit: 3 convolutions with BatchNorm + Scale, 1 ReLU behind conv1, the shuffle, Eltwise or Pooling + Concat, the ReLU
    assert count(s, "ShuffleChannel") == 16 and count(s, "Eltwise") == 13 and count(s, "Concat") == 3 and count(s, "Pooling") == 1 + 3 + 1
    depthwise = [l for l in s.layers if s.is_depthwise(l)]
    assert len(depthwise) == 16 and {l.type for l in depthwise} == {"Convolution" if dwt == "Convolution" else "DepthwiseConvolution"}
    assert count(s, "BatchNorm") == count(s, "Scale") == 1 + 16 * 3 and count(s, "ReLU") == 1 + 16 * 2
    assert len(s.layers) == 1 + 4 + 1 + 13 * 13 + 3 * 14 + 2 + extra      # data, conv1 (4), pool1, the units, pool_ave + fc1000, the ends
    B = s.blob_shapes
    assert B["conv1"] == (1, 24, 112, 112) and B["pool1"] == (1, 24, 56, 56)
    assert B["resx1_concat"] == (1, 240, 28, 28) and B["resx4_elewise"] == (1, 240, 28, 28) and B["resx5_concat"] == (1, 480, 14, 14)
    assert B["resx12_elewise"] == (1, 480, 14, 14) and B["resx13_concat"] == (1, 960, 7, 7) and B["resx16_elewise"] == (1, 960, 7, 7)
    assert B["resx1_conv1"] == B["shuffle1"] == (1, 60, 56, 56) and B["resx1_conv2"] == (1, 60, 28, 28) and B["resx1_conv3"] == (1, 216, 28, 28)
    assert B["resx1_match_conv"] == (1, 24, 28, 28) and B["resx5_conv3"] == (1, 240, 14, 14) and B["shuffle16"] == (1, 240, 7, 7)
    assert B["pool_ave"] == (1, 960, 1, 1) and B["fc1000"] == (1, 1000, 1, 1)
    groups = {l.name: int(l.sub("convolution_param").get("group", 1)) for l in s.layers if l.type == "Convolution" and not s.is_depthwise(l)}
    assert groups["resx1_conv1"] == 1 and groups["resx1_conv3"] == 3 and groups["resx2_conv1"] == 3 and groups["conv1"] == 1 and groups["fc1000"] == 1
    assert all(int(l.sub("shuffle_channel_param").get("group")) == 3 for l in s.layers if l.type == "ShuffleChannel")
    assert s.output_blobs() == {"DEPLOY": ["prob"], "TRAIN": ["loss"], "TEST": ["accuracy", "loss"]}[phase]
    assert "use_global_stats" in models.shufflenet_v1("DEPLOY") and "use_global_stats" not in models.shufflenet_v1("TRAIN")


@pytest.mark.parametrize("size,pads", [(224, ["", "", ""]), (64, ["", "", ""]), (200, ["", " pad: 1", " pad: 1"]), (108, [" pad: 1", "", " pad: 1"])])
def test_the_branches_of_a_stride_2_unit_agree_on_even_and_odd_edges(size, pads):
    txt = models.shufflenet_v1("DEPLOY", size=size)
    s = infer(txt, "DEPLOY")      # (a Concat whose bottoms disagree is refused by infer)
    for unit, pad in zip((1, 5, 13), pads):
        assert ('pooling_param { pool: AVE kernel_size: 3 stride: 2%s }' % pad) in txt.split('name: "resx%d_match_conv"' % unit)[1].split("}")[0] + "}"
        assert s.blob_shapes["resx%d_match_conv" % unit][2:] == s.blob_shapes["resx%d_conv3" % unit][2:]
    v2 = infer(models.shufflenet_v2("DEPLOY", size=size), "DEPLOY")
    assert v2.blob_shapes["stage2_1/left_conv"][2:] == v2.blob_shapes["stage2_1/conv2"][2:]


def test_shufflenet_v1_small_and_its_refused_groups_and_widths():
    s = infer(models.shufflenet_v1("TRAIN", **SMALL_V1), "TRAIN")
    B = s.blob_shapes
    assert B["conv1"] == (2, 12, 32, 32) and B["resx1_concat"] == (2, 48, 8, 8) and B["resx5_concat"] == (2, 96, 4, 4) and B["resx13_concat"] == (2, 192, 2, 2)
    assert B["shuffle1"] == (2, 12, 16, 16) and B["fc1000"] == (2, 10, 1, 1) and B["label"] == (2, 1, 1, 1)
    for l in s.layers:      # every group on whole 16-byte segments of floats
        g = int(l.sub("convolution_param").get("group", 1)) if l.type == "Convolution" and not s.is_depthwise(l) else 1
        if g > 1:
            cin, cout = B[l.bottoms[0]][1], B[l.tops[0]][1]
            assert (cin // g) % 4 == 0 and (cout // g) % 4 == 0, l.name
    for groups, n in ((2, 25), (4, 17), (8, 45)):
        with pytest.raises(ValueError, match=r"resx1_conv3 has \d+ (input|output) channels in %d groups: %d channels per group" % (groups, n)):
            models.shufflenet_v1("DEPLOY", groups=groups)
    with pytest.raises(ValueError, match="resx1_conv3 has 30 input channels in 3 groups: 10 channels per group"):
        models.shufflenet_v1("DEPLOY", width_div=2)
    with pytest.raises(ValueError, match="groups must be one of"):
        models.shufflenet_v1("DEPLOY", groups=5)
    with pytest.raises(ValueError, match="depthwise_type must be one of"):
        models.shufflenet_v1("DEPLOY", depthwise_type="DepthwiseConvolution")
    g1 = infer(models.shufflenet_v1("DEPLOY", groups=1), "DEPLOY")      # no grouped layer at all: the widths of the paper's first column
    assert g1.blob_shapes["resx1_concat"][1] == 144 and g1.blob_shapes["resx13_concat"][1] == 576
    assert "_filler" not in models.shufflenet_v1("TRAIN", fillers=False) and "weight_filler" in models.shufflenet_v1("TRAIN")


@pytest.mark.parametrize("phase,extra", [("DEPLOY", 1), ("TRAIN", 2), ("TEST", 3)])
@pytest.mark.parametrize("dwt", models.DEPTHWISE_TYPES)
@pytest.mark.parametrize("width,stages", [(0.5, (48, 96, 192)), (1.5, (176, 352, 704))])
def test_shufflenet_v2_layers_and_stage_shapes(phase, extra, dwt, width, stages):
    s = infer(models.shufflenet_v2(phase, width=width, depthwise_type=dwt), phase)
    assert count(s, "ShuffleChannel") == count(s, "Concat") == 16 and count(s, "Slice") == 13 and count(s, "Eltwise") == 0
    depthwise = [l for l in s.layers if s.is_depthwise(l)]
    assert len(depthwise) == 16 + 3 and {l.type for l in depthwise} == {"Convolution" if dwt == "Convolution" else "DepthwiseConvolution"}
    # stride-1 unit: Slice, 3 x (conv, bn, scale), 2 ReLUs, Concat, shuffle = 14; stride-2 unit: 5 x (conv, bn, scale), 3 ReLUs, Concat, shuffle = 20
    assert len(s.layers) == 1 + 4 + 1 + 13 * 14 + 3 * 20 + 4 + 2 + extra
    B = s.blob_shapes
    assert B["pool1"] == (1, 24, 56, 56)
    for stage, c, hw, last in zip((2, 3, 4), stages, (28, 14, 7), (4, 8, 4)):
        for b in (1, last):
            assert B["stage%d_%d/shuffle" % (stage, b)] == B["stage%d_%d/concat" % (stage, b)] == (1, c, hw, hw)
        assert B["stage%d_2/left" % stage] == B["stage%d_2/right" % stage] == B["stage%d_2/conv2" % stage] == (1, c // 2, hw, hw)
        assert B["stage%d_1/left_conv" % stage] == B["stage%d_1/conv2" % stage] == (1, c // 2, hw, hw)
    assert B["conv5"] == (1, 1024, 7, 7) and B["fc1000"] == (1, 1000, 1, 1)
    assert all(int(l.sub("shuffle_channel_param").get("group")) == 2 for l in s.layers if l.type == "ShuffleChannel")
    assert s.output_blobs() == {"DEPLOY": ["prob"], "TRAIN": ["loss"], "TEST": ["accuracy", "loss"]}[phase]


def test_shufflenet_v2_small_and_its_refused_widths():
    s = infer(models.shufflenet_v2("TRAIN", **SMALL_V2), "TRAIN")
    B = s.blob_shapes
    assert B["conv1"] == (2, 8, 32, 32) and B["stage2_4/shuffle"] == (2, 16, 8, 8) and B["stage3_8/shuffle"] == (2, 32, 4, 4)
    assert B["stage4_4/shuffle"] == (2, 64, 2, 2) and B["stage2_2/right"] == (2, 8, 8, 8) and B["fc1000"] == (2, 10, 1, 1)
    for width, n in ((1.0, 58), (2.0, 122)):
        with pytest.raises(ValueError, match="branches of %d: a branch is a channel window" % n):
            models.shufflenet_v2("DEPLOY", width=width)
    with pytest.raises(ValueError, match="the units of stage 2 have 12 channels, branches of 6"):
        models.shufflenet_v2("DEPLOY", width_div=4)
    with pytest.raises(ValueError, match="width must be one of"):
        models.shufflenet_v2("DEPLOY", width=0.25)
    with pytest.raises(ValueError, match="depthwise_type must be one of"):
        models.shufflenet_v2("DEPLOY", depthwise_type="Depthwise")


def test_a_hand_written_prototxt_of_a_refused_width_is_refused_by_the_window_rule(monkeypatch):
    """What the writers refuse up front, the existing 16-byte rules refuse by layer name where such a net is planned."""
    from plan_stub import engine_factory
    stub = engine_factory(monkeypatch, public=True)
    data = 'layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 1 dim: 116 dim: 4 dim: 4 } } }\n'
    unit = (data + 'layer { name: "sl" type: "Slice" bottom: "data" top: "l" top: "r" slice_param { axis: 1 slice_point: 58 } }\n'
            'layer { name: "c" type: "Concat" bottom: "r" bottom: "l" top: "c" }\n'
            'layer { name: "sh" type: "ShuffleChannel" bottom: "r" top: "y" shuffle_channel_param { group: 2 } }\n')
    e = stub(unit)      # (the Slice copies: a window at 58 would start off 16 bytes)
    assert "sl" in e.copy_slices and e.blobs["r"].coffset == 0
    sh = next(l for l in e.spec.layers if l.name == "sh")
    e.blobs["r"].coffset, e.blobs["r"].cstride = 58, 116
    with pytest.raises(NotImplementedError, match="ShuffleChannel sh: a channel window that is not 16-byte aligned"):
        e._fwd_shuffle(sh, [])
    grouped = (data + 'layer { name: "g" type: "Convolution" bottom: "data" top: "g" convolution_param { num_output: 100 kernel_size: 1 group: 2 } }\n')
    with pytest.raises(NotImplementedError, match="grouped Convolution g: group 2 leaves 58 input and 50 output channels per group"):
        stub(grouped)
