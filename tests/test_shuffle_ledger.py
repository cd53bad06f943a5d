"""The ledger of BackwardPlanner.shuffles (no GPU), by the rule tests/test_neuron_ledger.py holds the neurons table to.

The channel shuffle of csrc/shuffle.hip has a table of its own, the fifth, which _one_bottom consults after one_bottom, activations and
neurons.  Its one key - read from a planner built on a stub engine, not listed by hand - is the layer under test of the fan-out cases of
tests/test_gpu_shuffle_fanout.py (tests/torch_shuffle_ref.FANOUT), in nets where the launch accumulates and in nets where it does not; it
is a key of none of the four older tables, so the partitions of tests/test_backward_ledger.py, tests/test_act_ledger.py and
tests/test_neuron_ledger.py stand."""
import types

import pytest

from fcn_object_detector_amd import backward as BW
from fcn_object_detector_amd.netspec import ACT_TYPES, NEURON_TYPES, SHUFFLE_TYPES
from torch_shuffle_ref import FANOUT, fanout_case


@pytest.fixture
def planner(monkeypatch):
    monkeypatch.setattr(BW.L, "load", lambda: None)
    eng = types.SimpleNamespace(spec=None, blobs={}, grad_blobs={}, _conv_layer_meta={}, aux_dev={})
    return BW.BackwardPlanner(eng)


def test_the_one_key_is_the_layer_under_test_of_fan_out_cases_with_both_flags(planner):
    table = set(planner.shuffles)
    assert table == set(SHUFFLE_TYPES) == {"ShuffleChannel"}
    for t in table:
        flags = {acc for _txt, _layer, typ, acc in FANOUT.values() if typ == t}
        assert flags == {0, 1}, "%s: the fan-out nets run it with accumulate flags %s" % (t, sorted(flags))
    assert {typ for _txt, _layer, typ, _acc in FANOUT.values()} == table


def test_it_is_a_key_of_none_of_the_four_older_tables(planner):
    older = set(planner.emitters) | set(planner.one_bottom) | set(planner.activations) | set(planner.neurons)
    assert not set(planner.shuffles) & older
    assert all(callable(f) for f in planner.shuffles.values())
    assert set(planner.activations) == set(ACT_TYPES) and set(planner.neurons) == set(NEURON_TYPES)      # (those tables did not grow)


def test_the_layer_under_test_is_what_the_case_says():
    for name, (_txt, layer, typ, _acc) in FANOUT.items():
        spec, params, _x = fanout_case(name)
        l = next(q for q in spec.layers if q.name == layer)
        assert l.type == typ and layer not in params and l.tops[0] != l.bottoms[0], name
        c, g = spec.blob_shapes[l.bottoms[0]][1], int(l.sub("shuffle_channel_param").get("group"))
        assert g not in (1, c) and g * g != c, name      # never the identity, never self-inverse
    forms = set(FANOUT)
    assert {"behind_a_grouped_convolution_accumulates", "behind_a_grouped_convolution_writes_first", "behind_a_concat_of_two_branches_accumulates",
            "behind_a_concat_of_two_branches_writes_first", "in_front_of_a_slice_accumulates", "in_front_of_a_slice_alone", "on_a_2d_blob"} == forms
    spec, _p, _x = fanout_case("on_a_2d_blob")
    assert spec.blob_shapes["x"] == spec.blob_shapes["y"] == (2, 12)
    spec, _p, _x = fanout_case("behind_a_grouped_convolution_accumulates")
    assert int(next(l for l in spec.layers if l.name == "x").sub("convolution_param").get("group")) == 2
