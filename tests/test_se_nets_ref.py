"""The part of tests/test_gpu_se_nets.py that needs no GPU: its reference alone.

The gates of the seeded net spread over (0.1, 0.9) and differ between the two images; the reference run with the gate of image 0 for
both images misses the true one by far more than the float32 tolerance and the half-float one; the two forms are the same function of
the same weights; and the figure behind the half-float threshold - the float32 run of the rounded reference against the float64 one -
is measured again and stays within what that file records."""
import numpy as np
import torch

from conftest import rel_err
from torch_se_ref import BLOCKS, MEASURED_F32, TOL, TOL_F16, as_form, as_torch, gates_spread, half_reference, se_case, torch_se_net


def test_the_gates_spread_and_the_forms_agree():
    txt, spec, params, x = se_case("DEPLOY", "scale")
    atxt, aspec, _p, _x = se_case("DEPLOY", "axpy")
    assert "Axpy" in atxt and "Axpy" not in txt and [l.name for l in aspec.layers] == [l.name for l in spec.layers]
    with torch.no_grad():
        ref = torch_se_net(spec, as_torch(params), x)
        other = torch_se_net(aspec, as_torch(as_form(params, aspec)), x)
    gates_spread(ref)
    assert all(rel_err(other[n].numpy().reshape(ref[n].shape), ref[n].numpy()) < 1e-12 for n in BLOCKS + ["prob"])


def test_the_gate_of_image_0_for_both_images_is_caught():
    txt, spec, params, x = se_case("DEPLOY", "scale")

    def first_row(l, top, y):
        return y[:1].expand_as(y).clone() if l.type == "Sigmoid" else y
    with torch.no_grad():
        ref = torch_se_net(spec, as_torch(params), x)
        wrong = torch_se_net(spec, as_torch(params), x, round_blob=first_row)
    for n in BLOCKS + ["prob"]:
        assert rel_err(wrong[n].numpy(), ref[n].numpy()) > 20 * TOL_F16 > 20 * TOL, n


def test_the_half_float_threshold_is_the_measured_one():
    worst = 0.0
    for form in ("scale", "axpy"):
        txt, spec, params, x = se_case("DEPLOY", form)
        a, half = half_reference(spec, params, x)
        b, _ = half_reference(spec, params, x, torch.float32)
        assert all(n + "_prob" not in half and n in half and n + "/scale" in half for n in BLOCKS)      # the gates stay float32
        worst = max([worst] + [rel_err(b[n].double().numpy(), a[n].numpy()) for n in BLOCKS + [k + "_prob" for k in BLOCKS] + ["prob"]])
    print("MEASURED_F32 %.3g" % worst)
    assert worst <= MEASURED_F32 and TOL_F16 == min(4 * MEASURED_F32, 5e-3)
