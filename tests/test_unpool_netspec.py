"""Pooling with a mask top and the Upsample layer in the net description: shapes and every refusal, by layer name (no GPU)."""
import pytest

from fcn_object_detector_amd import proto
from fcn_object_detector_amd.netspec import NetSpec

HEAD = 'input: "data" input_shape { dim: 2 dim: 6 dim: %d dim: %d }\n'
POOL = 'layer { name: "pool1" type: "Pooling" bottom: "data" top: "pool1" top: "pool1_mask" pooling_param { pool: MAX kernel_size: %d stride: %d%s } }\n'
UP = 'layer { name: "up1" type: "Upsample" bottom: "pool1" bottom: "pool1_mask" top: "up1" upsample_param { %s } }\n'


def net(h, w, up, k=2, s=2, pad=0, extra=""):
    return HEAD % (h, w) + POOL % (k, s, " pad: %d" % pad if pad else "") + UP % up + extra


def infer(text, phase="TEST"):
    spec = NetSpec(proto.parse_text(text), phase)
    return spec, spec.infer()


def test_the_mask_has_the_pooled_shape_and_is_listed():
    spec, shapes = infer(net(8, 12, "scale: 2"))
    assert shapes["pool1"] == shapes["pool1_mask"] == (2, 6, 4, 6) and shapes["up1"] == (2, 6, 8, 12)
    assert list(spec.mask_blobs) == ["pool1_mask"] and spec.mask_blobs["pool1_mask"].name == "pool1"
    assert spec.output_blobs() == ["up1"]
    # a pooling without a second top has no mask, as before
    spec, shapes = infer(HEAD % (8, 12) + 'layer { name: "p" type: "Pooling" bottom: "data" top: "p" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }')
    assert spec.mask_blobs == {} and shapes["p"] == (2, 6, 4, 6)


def test_the_size_rules():
    assert infer(net(8, 12, ""))[1]["up1"] == (2, 6, 8, 12)                                     # scale defaults to 2
    assert infer(net(7, 9, "upsample_h: 7 upsample_w: 9"))[1]["up1"] == (2, 6, 7, 9)            # ceil mode: 4 x 5 pooled
    assert infer(net(7, 9, "scale: 2 pad_out_h: 1 pad_out_w: 1"))[1]["up1"] == (2, 6, 7, 9)     # 4 * 2 - 1, 5 * 2 - 1
    assert infer(net(7, 10, "pad_out_h: 1"))[1]["up1"] == (2, 6, 7, 10)                         # each axis has its own pad
    assert infer(net(7, 9, "scale: 2 upsample_h: 7 upsample_w: 9"))[1]["up1"] == (2, 6, 7, 9)   # the explicit extents win over the scale
    assert infer(net(9, 9, "scale: 3", k=3, s=3))[1]["up1"] == (2, 6, 9, 9)
    assert infer(net(7, 9, "upsample_h: 7 upsample_w: 9", k=3, s=2, pad=1))[1]["up1"] == (2, 6, 7, 9)
    # two Upsample layers may read one mask
    two = net(8, 12, "scale: 2") + UP.replace("up1", "up1b") % "scale: 2"
    assert infer(two)[1]["up1b"] == (2, 6, 8, 12)


def test_one_of_upsample_h_and_upsample_w_alone():
    with pytest.raises(ValueError, match="layer up1: Upsample with upsample_h and no upsample_w"):
        infer(net(7, 9, "upsample_h: 7"))
    with pytest.raises(ValueError, match="layer up1: Upsample with upsample_w and no upsample_h"):
        infer(net(7, 9, "upsample_w: 9"))


def test_bottoms_must_agree():
    text = net(8, 12, "scale: 2").replace('bottom: "pool1" bottom: "pool1_mask"', 'bottom: "data" bottom: "pool1_mask"')
    with pytest.raises(ValueError, match="layer up1: Upsample bottoms disagree"):
        infer(text)
    with pytest.raises(ValueError, match="layer up1: Upsample takes two 4-d bottoms"):
        infer(net(8, 12, "scale: 2").replace(' bottom: "pool1_mask" top: "up1"', ' top: "up1"'))


@pytest.mark.parametrize("param, what", [("pool: AVE kernel_size: 2 stride: 2", "AVE"), ("pool: MAX global_pooling: true", "global"),
                                         ("pool: STOCHASTIC kernel_size: 2 stride: 2", "STOCHASTIC")])
def test_only_max_pooling_writes_a_mask(param, what):
    text = HEAD % (8, 12) + 'layer { name: "pool1" type: "Pooling" bottom: "data" top: "pool1" top: "pool1_mask" pooling_param { %s } }' % param
    with pytest.raises(NotImplementedError, match="layer pool1: a second top .the mask pool1_mask. on %s pooling" % what):
        infer(text)


def test_a_rectangular_masked_pooling_is_refused_as_any_rectangular_pooling():
    text = HEAD % (8, 12) + 'layer { name: "pool1" type: "Pooling" bottom: "data" top: "pool1" top: "m" pooling_param { pool: MAX kernel_h: 2 kernel_w: 3 stride: 2 } }'
    with pytest.raises(NotImplementedError, match="layer pool1: Pooling with kernel 2x3"):
        infer(text)


def test_a_mask_that_no_pooling_of_this_net_wrote():
    text = HEAD % (4, 6) + 'input: "m" input_shape { dim: 2 dim: 6 dim: 4 dim: 6 }\n' + \
        'layer { name: "up1" type: "Upsample" bottom: "data" bottom: "m" top: "up1" upsample_param { scale: 2 } }'
    with pytest.raises(NotImplementedError, match="layer up1: the mask m is not the second top of a MAX Pooling of this net"):
        infer(text)
    # the FIRST top of a pooling is no mask either
    text = net(8, 12, "scale: 2").replace('bottom: "pool1" bottom: "pool1_mask"', 'bottom: "pool1" bottom: "pool1"')
    with pytest.raises(NotImplementedError, match="layer up1: the mask pool1 is not the second top"):
        infer(text)


def test_a_top_that_is_not_the_plane_the_mask_indexes():
    with pytest.raises(NotImplementedError, match="layer up1: Upsample to 8 x 10, but the mask pool1_mask indexes the 7 x 9 bottom of pool1: "
                                                  "upsample_h: 7 upsample_w: 9 would match"):
        infer(net(7, 9, "scale: 2"))
    with pytest.raises(NotImplementedError, match="layer up1: Upsample to 12 x 18.*upsample_h: 8 upsample_w: 12 would match"):
        infer(net(8, 12, "scale: 3"))


@pytest.mark.parametrize("layer, what", [
    ('layer { name: "c" type: "Convolution" bottom: "pool1_mask" top: "c" convolution_param { num_output: 4 kernel_size: 1 } }', "a layer of type Convolution"),
    ('layer { name: "c" type: "ReLU" bottom: "pool1_mask" top: "pool1_mask" }', "a layer of type ReLU"),
    ('layer { name: "c" type: "Eltwise" bottom: "pool1" bottom: "pool1_mask" top: "c" }', "a layer of type Eltwise"),
    ('layer { name: "c" type: "Concat" bottom: "pool1" bottom: "pool1_mask" top: "c" }', "a layer of type Concat"),
    ('layer { name: "c" type: "Upsample" bottom: "pool1_mask" bottom: "pool1_mask" top: "c" }', "the first bottom of an Upsample"),
])
def test_a_mask_feeds_upsample_layers_only(layer, what):
    with pytest.raises(NotImplementedError, match="layer c: the pooling mask pool1_mask .second top of pool1. feeds %s" % what):
        infer(net(8, 12, "scale: 2", extra=layer))


def test_the_forks_bn_type():
    text = HEAD % (8, 12) + 'layer { name: "conv1_bn" type: "BN" bottom: "data" top: "data" bn_param { scale_filler { type: "constant" value: 1 } } }'
    with pytest.raises(NotImplementedError, match="layer type 'BN' .layer conv1_bn.*write BatchNorm \\+ Scale"):
        infer(text)


def test_phases_and_in_place():
    with pytest.raises(ValueError, match="layer up1: Upsample cannot run in place"):
        infer(net(8, 12, "scale: 2").replace('top: "up1"', 'top: "pool1"'))
    with pytest.raises(ValueError, match="layer pool1: the mask top data must be a blob of its own"):
        infer(net(8, 12, "scale: 2").replace('top: "pool1_mask"', 'top: "data"'))
    spec, shapes = infer(net(8, 12, "scale: 2"), "TRAIN")
    assert shapes["up1"] == (2, 6, 8, 12) and "pool1_mask" in spec.mask_blobs
