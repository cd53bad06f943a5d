"""The ledger of BackwardPlanner.neurons (no GPU), by the rule tests/test_act_ledger.py holds the activations table to.

The parameter-free activations of csrc/neuron.hip have a table of their own, which _one_bottom consults after one_bottom and activations.
Every key of it - read from a planner built on a stub engine, not listed by hand - is the layer under test of a fan-out case of
tests/test_gpu_neuron_fanout.py (tests/torch_neuron_ref.FANOUT), in a net where the launch accumulates and in one where it does not; none
of them is a key of the three older tables, so the partitions of tests/test_backward_ledger.py and tests/test_act_ledger.py stand."""
import types

import pytest

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd.netspec import ACT_TYPES, NEURON_TYPES
from torch_neuron_ref import FANOUT, fanout_case


@pytest.fixture
def planner(monkeypatch):
    monkeypatch.setattr(BW.L, "load", lambda: None)
    eng = types.SimpleNamespace(spec=None, blobs={}, grad_blobs={}, _conv_layer_meta={}, aux_dev={})
    return BW.BackwardPlanner(eng)


def test_every_neuron_is_the_layer_under_test_of_a_fan_out_case(planner):
    table = set(planner.neurons)
    assert table == set(NEURON_TYPES) == {"ELU", "ReLU6", "Clip", "AbsVal", "BNLL", "Swish"}
    for t in table:
        flags = {acc for _txt, _layer, typ, acc in FANOUT.values() if typ == t}
        assert flags == {0, 1}, "%s: the fan-out nets run it with accumulate flags %s" % (t, sorted(flags))
    assert {typ for _txt, _layer, typ, _acc in FANOUT.values()} == table


def test_none_of_them_is_a_key_of_the_three_older_tables(planner):
    assert not set(planner.neurons) & (set(planner.emitters) | set(planner.one_bottom) | set(planner.activations))
    assert all(callable(f) for f in planner.neurons.values())
    assert set(planner.activations) == set(ACT_TYPES)      # (that table did not grow)


def test_the_layer_under_test_is_what_the_case_says():
    for name, (_txt, layer, typ, _acc) in FANOUT.items():
        spec, params, _x = fanout_case(name)
        l = next(q for q in spec.layers if q.name == layer)
        assert l.type == typ and layer not in params, name
    forms = set(FANOUT)
    for t in ("elu", "relu6", "swish"):
        assert {t + "_in_place_behind_a_convolution", t + "_in_place_behind_batchnorm_scale", t + "_in_place_behind_an_inner_product"} <= forms
    spec, _p, _x = fanout_case("swish_in_place_behind_an_inner_product")
    assert spec.blob_shapes["ip"] == (2, 12)      # a 2-d blob
    assert not any(n.startswith("absval_in_place") for n in forms)      # (refused by the NetSpec, as by Caffe)
