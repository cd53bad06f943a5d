"""The ledger of BackwardPlanner.activations (no GPU), by the rule tests/test_backward_ledger.py holds the two older tables to.

The one-bottom activations of csrc/act.hip have a table of their own, which _one_bottom consults where one_bottom has no entry.  Every key
of it - read from a planner built on a stub engine, not listed by hand - is the layer under test of a fan-out case of
tests/test_gpu_act_fanout.py (tests/torch_act_ref.FANOUT), in a net where the launch accumulates and in one where it does not; none of
them is a key of the two older tables, so the partition of tests/test_backward_ledger.py stands as it is."""
import types

import pytest

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd.netspec import ACT_TYPES
from torch_act_ref import FANOUT, fanout_case


@pytest.fixture
def planner(monkeypatch):
    monkeypatch.setattr(BW.L, "load", lambda: None)
    eng = types.SimpleNamespace(spec=None, blobs={}, grad_blobs={}, _conv_layer_meta={}, aux_dev={})
    return BW.BackwardPlanner(eng)


def test_every_activation_is_the_layer_under_test_of_a_fan_out_case(planner):
    table = set(planner.activations)
    assert table == set(ACT_TYPES)
    for t in table:
        flags = {acc for _txt, _layer, typ, acc in FANOUT.values() if typ == t}
        assert flags == {0, 1}, "%s: the fan-out nets run it with accumulate flags %s" % (t, sorted(flags))
    assert {typ for _txt, _layer, typ, _acc in FANOUT.values()} == table


def test_none_of_them_is_a_key_of_the_two_older_tables(planner):
    assert not set(planner.activations) & (set(planner.emitters) | set(planner.one_bottom))
    assert all(callable(f) for f in planner.activations.values())


def test_the_layer_under_test_is_what_the_case_says():
    for name, (_txt, layer, typ, _acc) in FANOUT.items():
        spec, params, _x = fanout_case(name)
        l = next(q for q in spec.layers if q.name == layer)
        assert l.type == typ, name
        assert (layer in params) == (typ != "TanH"), name
    forms = set(FANOUT)
    assert {"prelu_in_place_behind_a_convolution", "prelu_in_place_behind_batchnorm_scale", "prelu_in_place_behind_an_inner_product",
            "prelu_frozen", "prelu_channel_shared"} <= forms
    spec, _p, _x = fanout_case("prelu_in_place_behind_an_inner_product")
    assert spec.blob_shapes["ip"] == (2, 12)      # a 2-d blob
    spec, params, _x = fanout_case("prelu_channel_shared")
    assert params["act"][0].shape == () and float(params["act"][0]) != 0.0
    spec, _p, _x = fanout_case("prelu_frozen")
    assert next(q for q in spec.layers if q.name == "act").lr_mult == [0.0]
