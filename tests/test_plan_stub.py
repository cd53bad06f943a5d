"""The two seams the plan tests stand on - without a GPU.

Engine._init_state / TrainEngine._init_state declare the host-side state and touch no device; every slot that _adopt_backward fills and
_bn_ws exist from there on; the stub engine of tests/plan_stub.py keeps a pooling mask out of the outputs as Engine.__init__ does;
NetSpec.public is the keyword form the public entry points wrote out until it existed; a bare NetSpec refuses the newer layers as before."""
import inspect

import pytest

from fcn_object_detector_amd import engine as E
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import proto
from fcn_object_detector_amd import train as T
from fcn_object_detector_amd.netspec import FEATURES, NetSpec
from plan_stub import blank, engine_factory

DATA = 'layer { name: "data" type: "Input" top: "data" input_param { shape { dim: 2 dim: 3 dim: 4 dim: 4 } } }\n'
CONV = 'layer { name: "c" type: "Convolution" bottom: "data" top: "c" convolution_param { num_output: 8 kernel_size: 3 pad: 1 } }\n'
RELU = 'layer { name: "r" type: "ReLU" bottom: "c" top: "r" }\n'
LOSS = ('layer { name: "target" type: "Input" top: "target" input_param { shape { dim: 2 dim: 8 dim: 4 dim: 4 } } }\n'
        'layer { name: "loss" type: "EuclideanLoss" bottom: "c" bottom: "target" top: "loss" }\n')
MASKED = 'layer { name: "pool" type: "Pooling" bottom: "c" top: "pool" top: "pool_mask" pooling_param { pool: MAX kernel_size: 2 stride: 2 } }\n'
# what _adopt_backward assigns (test_adopt_backward_fills_declared_slots_only holds the list to the method)
BACKWARD_SLOTS = ("bwd_ops", "_ws", "_ip_ws", "_ip_wgrad_ws", "_gate_ws", "_act_ws", "_flip_flat", "_flip_segs_dev", "_tbank")


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError("_init_state touched the device: %r" % (a[:1],))
    monkeypatch.setattr(L, "call", refuse)
    monkeypatch.setattr(L, "load", refuse)
    for mod in (E, T):
        monkeypatch.setattr(mod, "DeviceBuffer", refuse)
        monkeypatch.setattr(mod, "PinnedArray", refuse)


def test_init_state_touches_no_device(no_device):
    e = blank(E.Engine, NetSpec(proto.parse_text(DATA + CONV + RELU), "TEST"))
    assert (e.inputs, e.outputs, e.shapes["r"]) == (["data"], ["r"], (2, 8, 4, 4))
    assert e.stream is None and not e.f16 and e.fuse and e.group_convs and e.autotune and not e.score_outputs
    assert (e.blobs, e.ops, e._group_workspaces, e._bn_chains, e._bn_ws_bytes, e._bn_ws) == ({}, [], [], {}, 0, None)
    assert blank(E.Engine, NetSpec(proto.parse_text(DATA + CONV + RELU), "TEST"), dtype="f16", fuse=False).f16
    solver = T.SolverParams(base_lr=0.5)
    t = blank(T.TrainEngine, NetSpec(proto.parse_text(DATA + CONV + LOSS), "TRAIN"), solver=solver, autotune=False)
    assert t.solver is solver and t.comm is None and (t.grad_blobs, t.bwd_ops, t.iter) == ({}, [], 0) and not t.autotune
    assert t.inputs == ["data", "target"] and t.outputs == ["loss"] and t.stream is None
    # the argument checks that need no device are made here
    with pytest.raises(ValueError, match="dtype must be 'f32' or 'f16'"):
        blank(E.Engine, NetSpec(proto.parse_text(DATA + CONV), "TEST"), dtype="bf16")
    with pytest.raises(NotImplementedError, match="the half-float path is inference only"):
        blank(E.Engine, NetSpec(proto.parse_text(DATA + CONV + LOSS), "TRAIN"), dtype="f16")
    with pytest.raises(ValueError, match="TrainEngine needs a TRAIN-phase NetSpec"):
        blank(T.TrainEngine, NetSpec(proto.parse_text(DATA + CONV), "TEST"))


def test_every_backward_slot_exists_before_a_planner_runs(monkeypatch):
    e = engine_factory(monkeypatch, backward=False)(DATA + CONV + LOSS, "TRAIN")
    have = vars(e)
    assert all(k in have for k in BACKWARD_SLOTS + ("_bn_ws",)), [k for k in BACKWARD_SLOTS + ("_bn_ws",) if k not in have]
    assert all(have[k] is None for k in BACKWARD_SLOTS[1:]) and have["bwd_ops"] == [] and have["_bn_ws"] is None


def test_adopt_backward_fills_declared_slots_only(monkeypatch):
    """_adopt_backward creates no attribute: whatever it takes off the planner, _init_state has declared."""
    make = engine_factory(monkeypatch, backward=False)
    e = make(DATA + CONV + LOSS, "TRAIN")
    before = set(vars(e))
    done = make(DATA + CONV + LOSS, "TRAIN", backward=True)
    assert set(vars(done)) - {"plan"} == before
    assert done.bwd_ops is done.plan.ops and done.bwd_ops and done._ws is done.plan.ws and done._flip_flat is done.plan.flip_flat
    assert set(BACKWARD_SLOTS) <= before
    src = inspect.getsource(T.TrainEngine._adopt_backward)
    assert all("self.%s" % k in src for k in BACKWARD_SLOTS)


def test_an_unread_pooling_mask_is_no_output(monkeypatch):
    e = engine_factory(monkeypatch)(DATA + CONV + MASKED)
    assert e.spec.output_blobs() == ["pool", "pool_mask"] and "pool_mask" in e.spec.mask_blobs and "pool_mask" in e.shapes
    assert e.outputs == ["pool"] and "pool_mask" not in e.blobs      # as Engine.__init__: the mask is the argmax buffer, not a blob


@pytest.mark.parametrize("phase", ["TRAIN", "TEST"])
def test_public_is_the_keyword_form_of_the_entry_points(phase):
    msg = proto.parse_text(DATA + CONV)
    explicit = NetSpec(msg, phase, depthwise=True, ip_gemm=True, rconv_f16=phase == "TEST", tconv_f16=phase == "TEST", scale_gate=True,
                       activations=True)
    public, bare = NetSpec.public(msg, phase), NetSpec(msg, phase)
    assert FEATURES == ("depthwise", "ip_gemm", "rconv_f16", "tconv_f16", "scale_gate", "activations")
    assert [getattr(public, k) for k in FEATURES] == [getattr(explicit, k) for k in FEATURES]
    assert [getattr(public, k) for k in FEATURES] == [True, True, phase == "TEST", phase == "TEST", True, True]
    assert public.phase == phase and [l.name for l in public.layers] == [l.name for l in explicit.layers]
    assert not any(getattr(bare, k) for k in FEATURES)
    # FEATURES names every opt-in keyword of the constructor and of from_file: a new one is added in all three places
    for fn in (NetSpec.__init__, NetSpec.from_file):
        assert tuple(k for k in inspect.signature(fn).parameters if k not in ("self", "msg", "path", "phase")) == FEATURES
    assert NetSpec.public_features(phase) == {k: getattr(explicit, k) for k in FEATURES}


def test_a_bare_netspec_still_refuses_by_name():
    prelu = DATA + CONV + 'layer { name: "p" type: "PReLU" bottom: "c" top: "c" }\n'
    with pytest.raises(NotImplementedError) as ei:
        NetSpec(proto.parse_text(prelu), "TEST").infer()
    assert str(ei.value) == ("layer type 'PReLU' (layer p): taken by a NetSpec built with activations=True (caffe.Net, the solvers and the caffe "
                             "tool pass it)")
    gate = DATA + CONV + ('layer { name: "g" type: "InnerProduct" bottom: "c" top: "g" inner_product_param { num_output: 8 } }\n'
                          'layer { name: "s" type: "Scale" bottom: "c" bottom: "g" top: "s" scale_param { axis: 0 } }\n')
    with pytest.raises(NotImplementedError) as ei:
        NetSpec(proto.parse_text(gate), "TEST").infer()
    assert str(ei.value) == ("layer s: Scale with two bottoms (the multiplier as a blob of the net): a per-image, per-channel gate over axis 0 is "
                             "taken by a NetSpec built with scale_gate=True (caffe.Net, the solvers and the caffe tool pass it)")
    for text in (prelu, gate):
        assert NetSpec.public(proto.parse_text(text), "TEST").infer()
