"""The reference's own nets are planned exactly as before grouped Convolution, InnerProduct backward and AVE-pooling backward arrived, -m gpu.

tests/golden/reference_oplists.json holds the forward and backward op lists - (kind, name) of every launch, the names carry the tile
configuration and the workgroup count the heuristics chose - of the three reference training nets at the test suites' sizes and of the
deploy net in both element types, recorded from the commit before that change with the autotuner off.  The layer graphs themselves are
held through tests/graph_signature.py: every Convolution of these nets is group 1, none has an InnerProduct or an AVE pooling that
needs a gradient, so none of the new planner branches may show."""
import json
import os

import pytest

from conftest import GOLDEN
from fcn_object_detector_amd import models, proto
from fcn_object_detector_amd.engine import Engine
from fcn_object_detector_amd.netspec import NetSpec, fill_params
from fcn_object_detector_amd.train import SolverParams, TrainEngine
from graph_signature import layer_digests, signature
from test_gpu_tconv_net import _reference_train_net

pytestmark = pytest.mark.gpu
NEW_KINDS = {"inner_product_bwd", "avepool_bwd"}


def _golden():
    return json.load(open(os.path.join(GOLDEN, "reference_oplists.json")))


def _lists(eng):
    return {"fwd": [[op.kind, op.name] for op in eng.ops], "bwd": [[op.kind, op.name] for op in getattr(eng, "bwd_ops", [])]}


@pytest.mark.parametrize("which", ["googlenet_detectnet_train", "fcn_bbox", "bounding_box"])
def test_training_plans_of_the_reference_nets(gpu, which):
    txt, shapes = _reference_train_net(which)
    msg = proto.parse_text(txt)
    _, layers = signature(msg, "TRAIN")
    assert len(layer_digests(layers)) == len(layers) and not any(l[0] == "InnerProduct" for l in layers)
    for l in layers:      # (type, name, ..., ("convolution_param", items), ...)
        for key, items in (x for x in l[7:] if isinstance(x, tuple) and len(x) == 2 and x[0] == "convolution_param"):
            assert l[0] == "Deconvolution" or dict(items).get("group", (1.0,)) == (1.0,), l[1]
    spec = NetSpec(msg, "TRAIN")
    spec.infer(shapes)
    sp = SolverParams(base_lr=0.0, momentum=0.0, weight_decay=0.0, lr_policy="fixed", solver_type="SGD")
    eng = TrainEngine(NetSpec(msg, "TRAIN"), shapes, params=fill_params(spec, seed=0), device=0, solver=sp, autotune=False)
    got = _lists(eng)
    eng.close()
    assert not NEW_KINDS & {k for k, _ in got["bwd"]}
    assert got["fwd"] == _golden()[which]["fwd"]
    assert got["bwd"] == _golden()[which]["bwd"]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_forward_plan_of_the_deploy_net(gpu, dtype):
    msg = proto.parse_text(models.googlenet_detectnet_deploy(1, 448, 448))
    spec = NetSpec(msg, "TEST")
    spec.infer()
    eng = Engine(NetSpec(msg, "TEST"), params=fill_params(spec, seed=0), device=0, autotune=False, dtype=dtype)
    got = _lists(eng)
    eng.close()
    assert got["fwd"] == _golden()["googlenet_detectnet_deploy_" + dtype]["fwd"]
