"""The Interp layer in NetSpec and in models.deeplab_*: the size rule of DeepLab-Caffe's InterpLayer, its refusals by layer name, the
published snippets, and the `interp` option of the DeepLab emitters - no GPU."""
import hashlib

import pytest

from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.netspec import Layer, NetSpec, interp_size


def layer(param, name="up"):
    return Layer(proto.parse_text('name: "%s" type: "Interp" bottom: "x" top: "y" interp_param { %s }' % (name, param)))


def net(param, shape=(2, 5, 9, 9), bottoms=("x",), top="y", name="up"):
    txt = 'input: "x" input_shape { %s }\ninput: "z" input_shape { dim: 2 dim: 5 dim: 4 dim: 4 }\n' % " ".join("dim: %d" % d for d in shape)
    txt += 'layer { name: "%s" type: "Interp" %s top: "%s" interp_param { %s } }' % (name, " ".join('bottom: "%s"' % b for b in bottoms), top, param)
    spec = NetSpec(proto.parse_text(txt), "TEST")
    return spec.infer()


def test_the_size_rule():
    assert interp_size(layer("zoom_factor: 8"), 41, 41) == (321, 321, 0, 0)
    assert interp_size(layer("zoom_factor: 8"), 65, 33) == (513, 257, 0, 0)
    assert interp_size(layer("shrink_factor: 8 pad_beg: 0 pad_end: 0"), 321, 321) == (41, 41, 0, 0)
    assert interp_size(layer("shrink_factor: 8"), 320, 17) == (40, 3, 0, 0)                       # (He - 1) // 8 + 1
    assert interp_size(layer("pad_beg: -1 pad_end: -2 shrink_factor: 2 zoom_factor: 4"), 9, 9) == (9, 9, -1, -2)      # 6 -> 3 -> 9
    assert interp_size(layer("height: 12 width: 7"), 1, 6) == (12, 7, 0, 0)
    assert interp_size(layer("height: 12 width: 7 pad_end: -1"), 3, 6) == (12, 7, 0, -1)
    # a factor of 1 that is written out counts as given
    assert interp_size(layer("zoom_factor: 1"), 5, 6) == (5, 6, 0, 0) and interp_size(layer("shrink_factor: 1"), 5, 6) == (5, 6, 0, 0)
    assert interp_size(layer("zoom_factor: 2 height: 3 width: 3"), 5, 6) == (9, 11, 0, 0)          # a factor goes before height / width
    assert net("zoom_factor: 4")["y"] == (2, 5, 33, 33)


@pytest.mark.parametrize("param, h, w, what", [
    ("zoom_factor: 2 pad_beg: 1", 9, 9, "pad_beg 1"),
    ("zoom_factor: 2 pad_end: 2", 9, 9, "pad_end 2"),
    ("zoom_factor: 2 pad_beg: -4 pad_end: -5", 9, 9, "leave nothing"),
    ("zoom_factor: 2 pad_beg: -3", 9, 3, "leave nothing"),
    ("", 9, 9, "needs zoom_factor, shrink_factor or both height and width"),
    ("height: 4", 9, 9, "needs zoom_factor"),
    ("width: 4 pad_beg: 0", 9, 9, "needs zoom_factor"),
    ("zoom_factor: 0", 9, 9, "at least 1"),
    ("shrink_factor: -2", 9, 9, "at least 1"),
    ("shrink_factor: 2 zoom_factor: 0", 9, 9, "at least 1"),
    ("height: 0 width: 4", 9, 9, "output extents"),
    ("height: 4 width: -1", 9, 9, "output extents"),
])
def test_refusals_name_the_layer(param, h, w, what):
    with pytest.raises(ValueError, match=r"layer up: .*%s" % what):
        interp_size(layer(param), h, w)
    with pytest.raises(ValueError, match=r"layer up: .*%s" % what):
        net(param, (2, 5, h, w))


def test_refusals_of_the_blobs():
    with pytest.raises(NotImplementedError, match=r"layer up: Interp with two bottoms"):
        net("zoom_factor: 2", bottoms=("x", "z"))
    with pytest.raises(ValueError, match=r"layer up: Interp cannot run in place"):
        net("zoom_factor: 2", top="x")
    with pytest.raises(ValueError, match=r"layer up: Interp takes one 4-d bottom"):
        net("zoom_factor: 2", shape=(2, 5))
    with pytest.raises(ValueError, match=r"layer up: Interp takes one 4-d bottom"):
        net("zoom_factor: 2", bottoms=())


PUBLISHED = """
input: "fc8_voc12" input_shape { dim: 1 dim: 21 dim: 65 dim: 65 }
input: "label" input_shape { dim: 1 dim: 1 dim: 321 dim: 321 }
layer {
  bottom: "fc8_voc12"
  top: "fc8_interp"
  name: "fc8_interp"
  type: "Interp"
  interp_param {
    zoom_factor: 8
  }
}
layer {
  bottom: "label"
  top: "label_shrink"
  name: "label_shrink"
  type: "Interp"
  interp_param {
    shrink_factor: 8
    pad_beg: 0
    pad_end: 0
  }
}
"""


def test_the_published_snippets_parse():
    shapes = NetSpec(proto.parse_text(PUBLISHED), "TEST").infer()
    assert shapes["fc8_interp"] == (1, 21, 513, 513) and shapes["label_shrink"] == (1, 1, 41, 41)


# sha256 of the emitters' default text before the option existed
BEFORE = {("deeplab_largefov", "DEPLOY"): "cebc115aca9d9e71", ("deeplab_largefov", "TRAIN"): "7b2c20ed31185d1e", ("deeplab_largefov", "TEST"): "9fec355a2b76598a",
          ("deeplab_aspp", "DEPLOY"): "9af6f8a013abe2c3", ("deeplab_aspp", "TRAIN"): "007eb7c12d5c0b5a", ("deeplab_aspp", "TEST"): "4aeaeea05f9a973a"}


@pytest.mark.parametrize("fn", ["deeplab_largefov", "deeplab_aspp"])
@pytest.mark.parametrize("phase", ["DEPLOY", "TRAIN", "TEST"])
def test_without_the_option_the_text_is_unchanged(fn, phase):
    txt = getattr(models, fn)(phase)
    assert hashlib.sha256(txt.encode()).hexdigest()[:16] == BEFORE[(fn, phase)]
    assert getattr(models, fn)(phase, interp=False) == txt and "Interp" not in txt
    small = dict(batch=2, size=137, width_div=8, fc_div=8, num_classes=5)
    assert getattr(models, fn)(phase, interp=False, **small) == getattr(models, fn)(phase, **small)


@pytest.mark.parametrize("fn", ["deeplab_largefov", "deeplab_aspp"])
def test_with_the_option(fn):
    emit = getattr(models, fn)
    kw = dict(batch=2, size=73, width_div=8, fc_div=8, num_classes=5, interp=True)
    score = models.deeplab_score_size(73)
    assert score == 10
    spec = NetSpec(proto.parse_text(emit("DEPLOY", **kw)), "TEST")
    shapes = spec.infer()
    assert shapes["fc8_voc12"] == (2, 5, score, score) and shapes["fc8_interp"] == (2, 5, 73, 73) and spec.output_blobs() == ["fc8_interp"]
    last = spec.layers[-1]
    assert (last.name, last.type, last.bottoms, int(last.sub("interp_param").get("zoom_factor"))) == ("fc8_interp", "Interp", ["fc8_voc12"], 8)
    for phase in ("TRAIN", "TEST"):
        spec = NetSpec(proto.parse_text(emit(phase, **kw)), phase)
        shapes = spec.infer()
        assert shapes["data"] == (2, 3, 73, 73) and shapes["label"] == (2, 1, 73, 73) and shapes["label_shrink"] == (2, 1, score, score)
        by = {l.name: l for l in spec.layers}
        p = by["label_shrink"].sub("interp_param")
        assert by["label_shrink"].bottoms == ["label"] and (int(p.get("shrink_factor")), int(p.get("pad_beg")), int(p.get("pad_end"))) == (8, 0, 0)
        assert by["loss"].bottoms == ["fc8_voc12", "label_shrink"] and "fc8_interp" not in by
        assert ("accuracy" in by) == (phase == "TEST") and (phase != "TEST" or by["accuracy"].bottoms == ["fc8_voc12", "label_shrink"])
    full = NetSpec(proto.parse_text(emit("DEPLOY", interp=True)), "TEST").infer()
    assert full["fc8_voc12"] == (1, 21, 41, 41) and full["fc8_interp"] == (1, 21, 321, 321)
    for size in (72, 74, 80, 136, 200):
        for phase in ("DEPLOY", "TRAIN"):
            with pytest.raises(ValueError, match="size %d is not 1 modulo 8" % size):
                emit(phase, **dict(kw, size=size))
