"""Where every byte of a net lives on the device (fcn_object_detector_amd/storage.py), checked without one.

plan_blobs decides which blobs own a buffer and which are channel windows of another's; param_layout and pack / unpack decide how
each parameter blob lies in the flat parameter buffer.  All of it is pure, so everything here runs on the CPU.

Provenance of the literals: the counts, digests and spot values below were recorded from the code this module replaced -
Engine._plan_buffers and Engine._alloc_params (with _packed_weight) of commit c86699b, run on a stub object (Engine.__new__, given
spec / shapes / dtype / fuse / inputs / outputs) with lib.load replaced by a fake whose fcn_malloc hands out increasing addresses and
whose fcn_memcpy_h2d_async keeps the bytes it is given, parameters from fill_params(spec, seed=3).  Per net that gave: for every
blob (esize, cstride, coffset, root blob, bytes of the root's buffer, upload_shift, lazy_shift, rows); alias, shift, copy_concats,
copy_slices, _half_inputs; every param_layout entry; param_count; and the bytes copied to each parameter segment.  A digest is the
SHA-1 of the canonical JSON (sorted keys, no spaces) of those; `record` below builds the same structure from storage.py.  The three
refusals of the buffer planner were reproduced on the parent the same way, the messages are its own.

Nets: the shipped ones the engines run (GoogLeNet DetectNet deploy in f32 / f16 - with the half image, with FCN_F16_IMAGE=0, with
fuse off -, both VGG16 deploy nets, FCN-8s at 1/16 width in both phases, the three training nets at the test suites' batch shapes, a
CaffeNet tail at fc = 512), plus hand-written ones for the branches none of those reaches: a Slice whose tops are views (no shipped
net has one), (N,) labels beside score rows, a Concat of two InnerProduct tops written in place and one that is copied, and the two
nets the planner refuses for a view of another element size and for an alias cycle.  New with this module: unpack of a bank of
halves returns float32 in Caffe's layout (the parent's read_param read such a convolution bank as float32 words).
"""
import hashlib
import json

import numpy as np
import pytest

from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd import storage as S
from fcn_object_detector_amd.netspec import NetSpec, fill_params

TAIL = """
name: "tail"
input: "data"
input_shape { dim: %d dim: 3 dim: 27 dim: 27 }
layer { name: "conv1" type: "Convolution" bottom: "data" top: "conv1" convolution_param { num_output: 24 kernel_size: 5 stride: 2
  weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "relu1" type: "ReLU" bottom: "conv1" top: "conv1" }
layer { name: "conv5" type: "Convolution" bottom: "conv1" top: "conv5" convolution_param { num_output: %d kernel_size: 3 pad: 1
  weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "relu5" type: "ReLU" bottom: "conv5" top: "conv5" }
layer { name: "pool5" type: "Pooling" bottom: "conv5" top: "pool5" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }
layer { name: "fc6" type: "InnerProduct" bottom: "pool5" top: "fc6" inner_product_param { num_output: %d
  weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 } } }
layer { name: "relu6" type: "ReLU" bottom: "fc6" top: "fc6" }
layer { name: "drop6" type: "Dropout" bottom: "fc6" top: "fc6" dropout_param { dropout_ratio: 0.5 } }
layer { name: "fc7" type: "InnerProduct" bottom: "fc6" top: "fc7" inner_product_param { num_output: %d bias_term: %s
  weight_filler { type: "xavier" } } }
layer { name: "relu7" type: "ReLU" bottom: "fc7" top: "fc7" }
layer { name: "fc8" type: "InnerProduct" bottom: "fc7" top: "fc8" inner_product_param { num_output: %d
  weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.0 } } }
layer { name: "prob" type: "Softmax" bottom: "fc8" top: "prob" }
""" % (10, 256, 512, 512, "true", 100)

FILL = 'weight_filler { type: "xavier" } bias_filler { type: "constant" value: 0.1 }'

# a Slice whose tops are views: 16-byte offsets (0 and 8 floats / halves), read by Convolution, Pooling and Concat only
SLICE_VIEW = """
input: "data"
input_shape { dim: 2 dim: 3 dim: 12 dim: 12 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 20 kernel_size: 3 pad: 1 %s } }
layer { name: "sl" type: "Slice" bottom: "c0" top: "s0" top: "s1" slice_param { slice_point: 8 } }
layer { name: "c1" type: "Convolution" bottom: "s0" top: "c1" convolution_param { num_output: 8 kernel_size: 1 %s } }
layer { name: "p1" type: "Pooling" bottom: "s1" top: "p1" pooling_param { pool: MAX kernel_size: 3 stride: 1 pad: 1 } }
layer { name: "c2" type: "Convolution" bottom: "p1" top: "c2" convolution_param { num_output: 8 kernel_size: 1 %s } }
layer { name: "cat" type: "Concat" bottom: "c1" bottom: "c2" top: "cat" }
layer { name: "c3" type: "Convolution" bottom: "cat" top: "c3" convolution_param { num_output: 5 kernel_size: 1 %s } }
""" % (FILL, FILL, FILL, FILL)

# (N,) labels beside (N, C) scores (`rows`), InnerProduct banks over a bottom with pad channels (3 channels in pixels of 4 / 8, H*W = 16)
ROWS = """
input: "data"
input_shape { dim: 6 dim: 3 dim: 4 dim: 4 }
input: "label"
input_shape { dim: 6 }
input: "target"
input_shape { dim: 6 dim: 10 }
layer { name: "a" type: "InnerProduct" bottom: "data" top: "a" inner_product_param { num_output: 10 %s } }
layer { name: "b" type: "InnerProduct" bottom: "data" top: "b" inner_product_param { num_output: 10 bias_term: false weight_filler { type: "xavier" } } }
layer { name: "sum" type: "Eltwise" bottom: "a" bottom: "b" top: "s" eltwise_param { operation: SUM } }
layer { name: "sig" type: "Sigmoid" bottom: "s" top: "sg" }
layer { name: "pw" type: "Power" bottom: "s" top: "pw" power_param { power: 1 scale: 2 shift: 1 } }
layer { name: "prob" type: "Softmax" bottom: "s" top: "prob" }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "s" bottom: "label" top: "loss" }
layer { name: "acc" type: "Accuracy" bottom: "s" bottom: "label" top: "acc" }
layer { name: "l2" type: "EuclideanLoss" bottom: "s" bottom: "target" top: "l2" }
layer { name: "l1" type: "L1Loss" bottom: "sg" bottom: "target" top: "l1" }
""" % FILL

# a Concat of two (N, C) InnerProduct tops: members in place (8 + 12) or copied (10 + 6: not whole 16-byte groups)
IPCAT = """
input: "data"
input_shape { dim: 5 dim: 6 dim: 3 dim: 3 }
layer { name: "a" type: "InnerProduct" bottom: "data" top: "a" inner_product_param { num_output: %d FILL } }
layer { name: "relu_a" type: "ReLU" bottom: "a" top: "a" }
layer { name: "b" type: "InnerProduct" bottom: "data" top: "b" inner_product_param { num_output: %d FILL } }
layer { name: "cat" type: "Concat" bottom: "a" bottom: "b" top: "cat" }
layer { name: "o" type: "InnerProduct" bottom: "cat" top: "o" inner_product_param { num_output: 7 FILL } }
layer { name: "sl" type: "Slice" bottom: "o" top: "o0" top: "o1" slice_param { slice_point: 3 } }
""".replace("FILL", FILL)

# refused: in a half-float engine c0 stays float32 (a Sigmoid reads it) while its Slice tops, read by convolutions only, are halves
MIXED_VIEW = """
input: "data"
input_shape { dim: 1 dim: 3 dim: 8 dim: 8 }
layer { name: "c0" type: "Convolution" bottom: "data" top: "c0" convolution_param { num_output: 8 kernel_size: 3 pad: 1 %s } }
layer { name: "sig" type: "Sigmoid" bottom: "c0" top: "sg" }
layer { name: "sl" type: "Slice" bottom: "c0" top: "s0" top: "s1" slice_param { slice_point: 4 } }
layer { name: "c1" type: "Convolution" bottom: "s0" top: "c1" convolution_param { num_output: 4 kernel_size: 1 %s } }
layer { name: "c2" type: "Convolution" bottom: "s1" top: "c2" convolution_param { num_output: 4 kernel_size: 1 %s } }
""" % (FILL, FILL, FILL)

# refused: two test-time Dropout layers that name each other's blobs
CYCLE = """
input: "a"
input_shape { dim: 1 dim: 4 dim: 2 dim: 2 }
layer { name: "d1" type: "Dropout" bottom: "a" top: "b" }
layer { name: "d2" type: "Dropout" bottom: "b" top: "a" }
"""

G = (2, 6, 8)
GN_TRAIN = {"data": (2, 3, 96, 128), "coverage-label": (2, 1, 6, 8), "bbox-label": (2, 4, 6, 8), "size-block": (2, 4, 6, 8),
            "obj-block": (2, 4, 6, 8), "coverage-block": (2, 4, 6, 8)}
BLK = (2, 8, 8, 8)
BB_TRAIN = {"data": (2, 3, 64, 64), "bbox-label": BLK, "size-block": BLK, "obj-block": BLK, "coverage-block": BLK, "coverage-label": (2, 2, 8, 8)}


def cases():
    m = models
    return {
        "googlenet_detectnet_deploy f32 b1": (m.googlenet_detectnet_deploy(1), "TEST", None, "f32", True, True),
        "googlenet_detectnet_deploy f16 b32": (m.googlenet_detectnet_deploy(32), "TEST", None, "f16", True, True),
        "googlenet_detectnet_deploy f16 b1, float32 image": (m.googlenet_detectnet_deploy(1), "TEST", None, "f16", True, False),
        "googlenet_detectnet_deploy f32 b1, fuse off": (m.googlenet_detectnet_deploy(1), "TEST", None, "f32", False, True),
        "vgg16_fcn_bbox_deploy f16": (m.vgg16_fcn_bbox_deploy(1, 64, 64, 2), "TEST", None, "f16", True, True),
        "vgg16_bounding_box_deploy f32": (m.vgg16_bounding_box_deploy(1, 448, 448, 2), "TEST", None, "f32", True, True),
        "voc_fcn8s TEST /16": (m.voc_fcn8s("TEST", num_classes=5, shape=(1, 3, 64, 48), width_div=16, fc_div=128, fillers=True), "TEST", None, "f32", True, True),
        "voc_fcn8s TRAIN /16": (m.voc_fcn8s("TRAIN", num_classes=5, shape=(1, 3, 64, 48), width_div=16, fc_div=128, fillers=True), "TRAIN", None, "f32", True, True),
        "googlenet_detectnet_train": (m.googlenet_detectnet_train("m", "L", "unused", num_classes=1), "TRAIN", GN_TRAIN, "f32", True, True),
        "googlenet_detectnet_train_lmdb": (m.googlenet_detectnet_train_lmdb(), "TRAIN", {"data": (2, 3, 96, 128), "label": (2, 17, 6, 8)}, "f32", True, True),
        "vgg16_bounding_box_train": (m.vgg16_bounding_box_train("m", "L", "unused", num_classes=2), "TRAIN", BB_TRAIN, "f32", True, True),
        "caffenet tail f32": (TAIL, "TEST", None, "f32", True, True),
        "caffenet tail f16": (TAIL, "TEST", None, "f16", True, True),
        "viewable slice f32": (SLICE_VIEW, "TEST", None, "f32", True, True),
        "viewable slice f16": (SLICE_VIEW, "TEST", None, "f16", True, True),
        "rows labels f32": (ROWS, "TEST", None, "f32", True, True),
        "rows labels f16": (ROWS, "TEST", None, "f16", True, True),
        "inner product concat in place f32": (IPCAT % (8, 12), "TEST", None, "f32", True, True),
        "inner product concat in place f16": (IPCAT % (8, 16), "TEST", None, "f16", True, True),
        "inner product concat copied f32": (IPCAT % (10, 6), "TEST", None, "f32", True, True),
        "mixed view f16": (MIXED_VIEW, "TEST", None, "f16", True, True),
        "alias cycle": (CYCLE, "TEST", None, "f32", True, True),
    }


# name -> (blobs, views, parameter segments, param_count, digest of the blob plan, of the layout, of the SHA-1s of the segments' bytes)
PARENT = {
    "googlenet_detectnet_deploy f32 b1": (86, 38, 118, 5997188, "5521ba2222273bd5e4a55453fa1d22641850e13b", "59355f5619435c46387cb070b2d92407247f2087", "1939f31986d09cd1d1c8c16871c6d1ce180df0f9"),
    "googlenet_detectnet_deploy f16 b32": (86, 38, 118, 3008516, "42c048481e35d2d1cea444ea631fee390136c908", "6bb883e1c53468f3897758b0b688278e11b87d7f", "8c154dd6d800f1f287250e7fd8a7210e2c8ecec4"),
    "googlenet_detectnet_deploy f16 b1, float32 image": (86, 38, 118, 3008516, "3403a07b2c59f2ad0d8cdde4cbfba5fa86455ba7", "98b06308525874d7daff5dc64d8ddc02d5270b4e", "cf214da202e9d621b886012ec6496909da6e5d35"),
    "googlenet_detectnet_deploy f32 b1, fuse off": (86, 1, 118, 5997188, "c5219d6a404ed7a246de0ae42fe84a4c83be1187", "59355f5619435c46387cb070b2d92407247f2087", "1939f31986d09cd1d1c8c16871c6d1ce180df0f9"),
    "vgg16_fcn_bbox_deploy f16": (31, 1, 38, 7365332, "06a01a801a9942d273a09498994fe83ff8f9d0f2", "d89353ac55b7a35f678155cce629ea813b0236bf", "290b40a246894bdb1b357f8475e16ad0220906fd"),
    "vgg16_bounding_box_deploy f32": (35, 1, 42, 15524876, "f1fef942872eb81cc14020df9406c41acff18be5", "801a9340f049aaf801150140bbd7a44e9e6ef9f9", "2c9a716e119e44c85dbc40e1f716b93a8f2a6579"),
    "voc_fcn8s TEST /16": (32, 0, 39, 121072, "609246bb5edba90bffa4dca04825d6e27ee1bdf2", "82d5eeb165288599d275ce304a710b0d9b8e9eb0", "64e8e93bea67a935d8c60cd56fb2790de6c21f2e"),
    "voc_fcn8s TRAIN /16": (34, 0, 39, 121072, "8059c878658b39b4b05b29ad519081856289a409", "82d5eeb165288599d275ce304a710b0d9b8e9eb0", "64e8e93bea67a935d8c60cd56fb2790de6c21f2e"),
    "googlenet_detectnet_train": (98, 37, 118, 5981816, "d3f13b80d1371c23a8f8b480de38eb6f6117ea10", "5094e35baf2d6b29b45fc9c2188d1551539dda18", "043dca3ade13e810959c7e9179aafa736d77d65b"),
    "googlenet_detectnet_train_lmdb": (99, 37, 118, 5981816, "3588b70f9553180559740910363a8b6345f8ab6f", "5094e35baf2d6b29b45fc9c2188d1551539dda18", "043dca3ade13e810959c7e9179aafa736d77d65b"),
    "vgg16_bounding_box_train": (35, 0, 31, 14728588, "8d987dacddfbe003a1bc0d7323f25ae67ad22914", "040c035acd7ceb2aa19c2385c92f1c208ad077ce", "95d8cbdda2de696ad4ca9624604b8bea908caa13"),
    "caffenet tail f32": (8, 0, 10, 5091036, "97b311feb023ea8ba8ae756d5e2ccd94b2c981e3", "8594912957d2016da3ae7b557e3957ba44efab78", "91e7a68d0351a33631be625e89a9bed38bef77c9"),
    "caffenet tail f16": (8, 0, 10, 2547420, "f6ffe2738ec887a9446f87066b793627417071ef", "7a79c933c14b06ddb2ccc57c43aefa71dad885b7", "365fb5571822a86703b01a6def6bf139d4bb8c2b"),
    "viewable slice f32": (9, 4, 8, 1004, "af93a08b35bf582cdd3753c7daa5f06622aae5a5", "6444f73b1a74a805862afc5a55a2d232f3378b3f", "159baab17d14f712784509235fc99f28bfd1ab49"),
    "viewable slice f16": (9, 4, 8, 900, "b05c9505918269192d3e572db5f3df2026a8c831", "5e19fb0b4873e52208ffbfad5fad9d8ec3bb38c2", "4330362c1edab504c682f51d6f2bf70e11c41509"),
    "rows labels f32": (13, 0, 3, 1292, "53823719e4114b49525b09335683ee1778e8b41a", "b2335369994ce03e6d2801edbdaec454ec7e485e", "68654fa26bdda7f4350d8e5a7d7db64f158f0ddd"),
    "inner product concat in place f32": (7, 2, 6, 1608, "40ec1cc627e80455c2b3ccaae2f04dacf45039ca", "058ac24a767a8a393a71672ca740a42cbd3dfb1a", "2f105f218560d5ba67bfd62fa3ca71f1dc16addb"),
    "inner product concat copied f32": (7, 0, 6, 1292, "51e937f2844bd114d8086bb974b9a5d2594f2cfb", "0667200537371e1044b10867ab25c416b74fc064", "240941559b3969910304f895ed517c1fbbbb9355"),
}
REFUSED = {
    "rows labels f16": (NotImplementedError, "f16 engine: float32 blob s is produced by ['Eltwise']"),
    "inner product concat in place f16": (NotImplementedError, "f16 engine: float32 blob o0 is produced by ['Slice']"),
    "mixed view f16": (NotImplementedError, "f16 engine: blob s0 (2-byte elements) is a view of c0 (4-byte)"),
    "alias cycle": (RuntimeError, "alias cycle at blob b"),
}


def plan_of(txt, phase="TEST", data_shapes=None, dtype="f32", fuse=True, half_image=True):
    spec = NetSpec(proto.parse_text(txt), phase)
    shapes = spec.infer(data_shapes)
    outputs = [b for b in spec.output_blobs() if b in shapes]
    return spec, S.plan_blobs(spec, shapes, spec.data_tops(), outputs, dtype == "f16", fuse, half_image)


def folded_shift(spec, plan, seg):
    """What Engine._folded_shift hands to pack: the shift of a half image, for the convolution that reads its Power top."""
    l = next(q for q in spec.layers if q.name == seg.layer)
    return next((sh for t, sh in plan.half_inputs.values() if seg.kind == S.CONV and t == l.bottoms[0]), 0.0)


def digest(obj):
    return hashlib.sha1(json.dumps(obj, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


_built = {}


def built(name):
    """(spec, plan, segments, param_count, parameters) of a recorded net, made once."""
    if name not in _built:
        txt, phase, data_shapes, dtype, fuse, half_image = cases()[name]
        spec, plan = plan_of(txt, phase, data_shapes, dtype, fuse, half_image)
        segs, count = S.param_layout(spec, plan.views, dtype == "f16")
        _built[name] = (spec, plan, segs, count, fill_params(spec, seed=3))
    return _built[name]


@pytest.mark.parametrize("name", sorted(PARENT))
def test_blob_plan_layout_and_packed_bytes_are_the_parents(name):
    spec, plan, segs, count, params = built(name)
    blobs, views, nsegs, param_count, plan_digest, layout_digest, bytes_digest = PARENT[name]
    assert (len(plan.views), len(plan.alias), len(segs), count) == (blobs, views, nsegs, param_count)
    rec = dict(blobs={n: [v.esize, v.cstride, v.coffset, v.root, plan.root_bytes[v.root], v.upload_shift, v.lazy_shift, v.rows]
                      for n, v in plan.views.items()},
               alias={k: list(v) for k, v in plan.alias.items()}, shift=plan.shift, copy_concats=sorted(plan.copy_concats),
               copy_slices=sorted(plan.copy_slices), half_inputs={k: list(v) for k, v in plan.half_inputs.items()})
    assert digest(rec) == plan_digest
    assert all(plan.esize[n] == v.esize and (n in plan.rows) == v.rows for n, v in plan.views.items())
    assert set(plan.root_bytes) == set(plan.views) - set(plan.alias)
    layout = [[s.layer, s.index, s.offset, s.count, list(s.shape), s.lr_mult, s.decay_mult, s.nbytes] for s in segs]
    assert digest(layout) == layout_digest
    sent = []
    for s in segs:
        arr = S.pack(s, params[s.layer][s.index], folded_shift(spec, plan, s))
        assert arr.flags["C_CONTIGUOUS"] and arr.shape == s.shape and arr.nbytes == s.nbytes and arr.size == s.count
        sent.append(hashlib.sha1(arr.tobytes()).hexdigest())
    assert digest(sent) == bytes_digest


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_the_planner_refuses_by_the_parents_words(name):
    txt, phase, data_shapes, dtype, fuse, half_image = cases()[name]
    kind, words = REFUSED[name]
    with pytest.raises(kind) as err:
        plan_of(txt, phase, data_shapes, dtype, fuse, half_image)
    assert str(err.value) == words


def test_spot_values_of_the_googlenet_deploy_plans():
    _spec, plan, segs, _count, _params = built("googlenet_detectnet_deploy f32 b1")
    v = plan.views
    # the Power(-127) on the input is folded into the upload: both names share the buffer, reading `data` back undoes the shift
    assert v["data"] == S.BlobView((1, 3, 448, 448), 4, "data", 0, 4, -127.0, 127.0, False)
    assert v["transformed_data"] == S.BlobView((1, 3, 448, 448), 4, "data", 0, 4, 0.0, 0.0, False)
    assert plan.shift == {"transformed_data": -127.0} and plan.half_inputs == {} and plan.root_bytes["data"] == 448 * 448 * 4 * 4
    # inception branches write their channel slice of the module's output; the test-time Dropout top is the pooled blob itself
    assert (v["inception_3a/3x3"].root, v["inception_3a/3x3"].coffset, v["inception_3a/3x3"].cstride) == ("inception_3a/output", 64, 256)
    assert (v["inception_3a/pool_proj"].root, v["inception_3a/pool_proj"].coffset) == ("inception_3a/output", 224)
    assert plan.alias["pool5/drop_s1"] == ("inception_5b/output", 0) and not plan.copy_concats and not plan.copy_slices
    assert segs[0] == S.ParamSeg("conv1/7x7_s2", 0, S.CONV, 0, 12544, (64, 7, 7, 4), (64, 3, 7, 7), 1.0, 1.0, 50176, 4)
    assert segs[1] == S.ParamSeg("conv1/7x7_s2", 1, S.PLAIN, 12544, 64, (64,), (64,), 2.0, 0.0, 256, 4)
    assert segs[2] == S.ParamSeg("conv2/3x3_reduce", 0, S.CONV, 12608, 4096, (64, 1, 1, 64), (64, 64, 1, 1), 1.0, 1.0, 16384, 4)

    spec, plan, segs, _count, params = built("googlenet_detectnet_deploy f16 b32")
    v = plan.views
    # the half image: un-shifted halves in pixels of 8, the Power top adds the shift when it is read; the first bank is halves too
    assert plan.half_inputs == {"data": ("transformed_data", -127.0)}
    assert v["data"] == S.BlobView((32, 3, 448, 448), 2, "data", 0, 8, 0.0, 0.0, False)
    assert v["transformed_data"] == S.BlobView((32, 3, 448, 448), 2, "data", 0, 8, 0.0, -127.0, False)
    assert plan.root_bytes["data"] == 102760448 and v["coverage"].esize == 4 and v["inception_3a/output"].esize == 2
    assert segs[0] == S.ParamSeg("conv1/7x7_s2", 0, S.CONV, 0, 25088, (64, 7, 7, 8), (64, 3, 7, 7), 1.0, 1.0, 50176, 2)
    assert segs[2] == S.ParamSeg("conv2/3x3_reduce", 0, S.CONV, 12608, 4096, (64, 1, 1, 64), (64, 64, 1, 1), 1.0, 1.0, 8192, 2)
    # the folded shift: channels 3 and 4 of the first bank carry -127 * sum_c(w_c) of the rounded filters as a half and its remainder
    w = params["conv1/7x7_s2"][0]
    bank = S.pack(segs[0], w, folded_shift(spec, plan, segs[0]))
    term = -127.0 * w.astype(np.float16).astype(np.float64).sum(1)
    assert bank.dtype == np.float16 and np.array_equal(bank[..., 3], term.astype(np.float16)) and not bank[..., 5:].any()
    assert np.abs(bank[..., 3].astype(np.float64) + bank[..., 4].astype(np.float64) - term).max() <= 2.0 ** -21 * np.abs(term).max()
    assert folded_shift(spec, plan, segs[2]) == 0.0

    _spec, plan, segs, _count, _params = built("googlenet_detectnet_deploy f16 b1, float32 image")
    assert plan.half_inputs == {} and plan.views["data"].esize == 4 and plan.views["data"].upload_shift == -127.0
    assert segs[0].esize == 4 and segs[0].shape == (64, 7, 7, 4) and segs[2].esize == 2


def test_spot_values_of_the_other_nets():
    _spec, plan, segs, _c, _p = built("googlenet_detectnet_train_lmdb")
    # the one copied Slice: the 17-channel label record cut at 1, 5, 9, 13 for Eltwise layers
    assert plan.copy_slices == {"slice-label"} and plan.views["label"].cstride == 20 and plan.views["bbox-label"].root == "bbox-label"
    assert "pool5/drop_s1" not in plan.alias                     # TRAIN: Dropout computes
    assert plan.views["loss_bbox"].nchw is None and plan.root_bytes["loss_bbox"] == 16
    _spec, plan, segs, _c, _p = built("vgg16_bounding_box_deploy f32")
    assert plan.copy_concats == {"conv4_3/conv5_3/concat"} and plan.alias == {"dropout5": ("conv4_3/conv5_3/concat", 0)}
    up = next(s for s in segs if s.layer == "conv4_3/7x7/upsample")
    assert (up.kind, up.offset, up.shape, up.host_shape, up.lr_mult) == (S.PLAIN, 8421888, (128, 8, 8), (128, 1, 8, 8), 0.0)      # depthwise
    _spec, plan, segs, _c, _p = built("voc_fcn8s TEST /16")
    up = next(s for s in segs if s.layer == "upscore8")
    assert (up.kind, up.offset, up.shape, up.host_shape, up.nbytes) == (S.DECONV, 110832, (5, 16, 16, 8), (5, 5, 16, 16), 40960)     # group 1
    _spec, plan, segs, _c, _p = built("caffenet tail f16")
    fc6 = next(s for s in segs if s.layer == "fc6" and s.index == 0)
    assert fc6 == S.ParamSeg("fc6", 0, S.INNER_PRODUCT, 30328, 4718592, (512, 9216), (512, 9216), 1.0, 1.0, 9437184, 2, (256, 6, 6, 256))
    assert plan.views["fc8"].shape == (10, 100) and plan.views["fc8"].cstride == 104 and plan.views["prob"].esize == 4
    _spec, plan, segs, _c, _p = built("rows labels f32")
    assert plan.rows == {"label"} and plan.views["label"].nchw == (6, 1, 1, 1) and plan.root_bytes["label"] == 96
    assert segs[0].bottom == (3, 4, 4, 4) and segs[0].shape == (10, 64) and segs[2].offset == 652
    _spec, plan, segs, _c, _p = built("viewable slice f16")
    assert plan.alias == {"s0": ("c0", 0), "s1": ("c0", 8), "c1": ("cat", 0), "c2": ("cat", 8)} and not plan.copy_slices
    assert plan.views["s1"] == S.BlobView((2, 12, 12, 12), 2, "c0", 8, 24, 0.0, 0.0, False)
    _spec, plan, segs, _c, _p = built("inner product concat in place f32")
    assert plan.alias == {"a": ("cat", 0), "b": ("cat", 8)} and plan.copy_slices == {"sl"} and plan.views["b"].cstride == 20
    assert built("inner product concat copied f32")[1].copy_concats == {"cat"}


# a bottom with pad channels under two InnerProduct layers: 6 channels in pixels of 8, 3 x 3 pixels, in both element types
IP_PAD = """
input: "data"
input_shape { dim: 2 dim: 5 dim: 5 dim: 5 }
layer { name: "c" type: "Convolution" bottom: "data" top: "c" convolution_param { num_output: 6 kernel_size: 3 %s } }
layer { name: "relu" type: "ReLU" bottom: "c" top: "c" }
layer { name: "c2" type: "Convolution" bottom: "c" top: "c2" convolution_param { num_output: 11 kernel_size: 1 %s } }
layer { name: "ip" type: "InnerProduct" bottom: "c" top: "ip" inner_product_param { num_output: 10 %s } }
layer { name: "ip2" type: "InnerProduct" bottom: "c2" top: "ip2" inner_product_param { num_output: 7 %s } }
""" % (FILL, FILL, FILL, FILL)


def round_trip(spec, plan, segs, params):
    for s in segs:
        w = params[s.layer][s.index]
        packed = S.pack(s, w, folded_shift(spec, plan, s))
        want = w.astype(np.float16).astype(np.float32) if s.esize == 2 else w
        for raw in (packed, np.frombuffer(packed.tobytes(), np.uint8), np.frombuffer(packed.tobytes() + b"\0" * (-s.nbytes % 4), np.float32)):
            got = S.unpack(s, raw)           # the device array, its bytes (read_param), its words (a slice of the flat buffer)
            assert got.dtype == np.float32 and got.shape == s.host_shape and got.flags["C_CONTIGUOUS"], (s.layer, s.index)
            assert np.array_equal(got, want), (s.layer, s.index)
        assert not np.shares_memory(S.unpack(s, packed), packed)


@pytest.mark.parametrize("name", sorted(PARENT))
def test_unpack_inverts_pack_on_every_segment_of_the_recorded_nets(name):
    spec, plan, segs, _count, params = built(name)
    round_trip(spec, plan, segs, params)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_unpack_inverts_pack_over_pad_channels(dtype):
    """Cin 5 (not whole groups of 4), 6 (not of 8), an InnerProduct bottom with cstride 8 over 6 channels and 3 x 3 pixels, one with
    cstride 12 / 16 over 11 channels."""
    spec, plan = plan_of(IP_PAD, dtype=dtype)
    segs, _count = S.param_layout(spec, plan.views, dtype == "f16")
    by = {(s.layer, s.index): s for s in segs}
    half = dtype == "f16"
    assert by[("c", 0)].shape == (6, 3, 3, 8) and by[("c", 0)].esize == 4                # the image is float32 in both
    assert by[("c2", 0)].shape == (11, 1, 1, 8) and by[("c2", 0)].esize == (2 if half else 4)
    assert by[("ip", 0)].bottom == (6, 3, 3, 8) and by[("ip", 0)].shape == (10, 72) and by[("ip", 0)].host_shape == (10, 54)
    assert by[("ip2", 0)].bottom == (11, 3, 3, 16 if half else 12) and by[("ip2", 0)].esize == (2 if half else 4)
    params = fill_params(spec, seed=9)
    round_trip(spec, plan, segs, params)
    bank = S.pack(by[("ip", 0)], params["ip"][0])          # column p * cstride + ch holds Caffe's column ch * H*W + p
    assert bank[4, 5 * 8 + 2] == np.asarray(params["ip"][0][4, 2 * 9 + 5], bank.dtype) and not bank.reshape(10, 9, 8)[:, :, 6:].any()


DECONV = """
input: "data"
input_shape { dim: 1 dim: 6 dim: 4 dim: 4 }
layer { name: "up" type: "Deconvolution" bottom: "data" top: "up" convolution_param { num_output: %d group: %d kernel_size: 4 stride: 2 bias_term: false } }
"""


def test_the_deconvolution_kind_is_decided_once():
    def layout(co, group, dtype="f32"):
        spec, plan = plan_of(DECONV % (co, group), dtype=dtype)
        return S.param_layout(spec, plan.views, dtype == "f16")[0]
    assert [(s.kind, s.shape, s.host_shape) for s in layout(6, 6)] == [(S.PLAIN, (6, 4, 4), (6, 1, 4, 4))]
    assert [(s.kind, s.shape, s.host_shape) for s in layout(6, 6, "f16")] == [(S.PLAIN, (6, 4, 4), (6, 1, 4, 4))]
    assert [(s.kind, s.shape, s.host_shape) for s in layout(5, 1)] == [(S.DECONV, (6, 4, 4, 8), (6, 5, 4, 4))]
    with pytest.raises(NotImplementedError) as err:
        layout(5, 1, "f16")
    assert str(err.value) == "f16 engine: layer type Deconvolution with group 1 (up) has no half-float kernel"
    with pytest.raises(NotImplementedError) as err:
        layout(6, 2)
    assert str(err.value) == "Deconvolution up: group 2 with 6 -> 6 channels (only group 1 and group == channels == num_output)"


def test_an_inner_product_over_a_channel_window_is_refused():
    txt = IPCAT % (8, 12) + 'layer { name: "w" type: "InnerProduct" bottom: "o0" top: "w" inner_product_param { num_output: 2 %s } }\n' % FILL
    txt = txt.replace('top: "o1" slice_param { slice_point: 3 }', 'top: "o1" slice_param { slice_point: 4 }')
    spec, plan = plan_of(txt)
    assert plan.alias["a"] == ("cat", 0) and plan.copy_slices == {"sl"}           # (an InnerProduct reads o0: the Slice copies)
    S.param_layout(spec, plan.views, False)
    txt = IPCAT % (8, 12) + 'layer { name: "w" type: "InnerProduct" bottom: "a" top: "w" inner_product_param { num_output: 2 %s } }\n' % FILL
    spec, plan = plan_of(txt)
    assert plan.copy_concats == {"cat"}                                           # a second reader: the Concat copies, `a` is whole
    S.param_layout(spec, plan.views, False)
    views = dict(plan.views, a=S.BlobView((5, 8), 4, "cat", 0, 20, 0.0, 0.0, False))
    with pytest.raises(NotImplementedError) as err:
        S.param_layout(spec, views, False)
    assert str(err.value) == "InnerProduct w: the bottom a is a channel window of a wider buffer (or no 4-d / 2-d blob)"


def test_shared_layers_are_skipped():
    spec, plan, segs, count, _params = built("viewable slice f32")
    rest, n = S.param_layout(spec, plan.views, False, skip={"c0"})
    assert [(s.layer, s.index) for s in rest] == [(s.layer, s.index) for s in segs if s.layer != "c0"]
    assert rest[0].offset == 0 and n == count - segs[2].offset
