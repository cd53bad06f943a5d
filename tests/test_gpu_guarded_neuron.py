"""The entry points of csrc/neuron.hip (ELU, Clip / ReLU6, AbsVal, BNLL, Swish) in guard-banded, poisoned buffers against
tests/ref_neuron64.py, -m gpu.

Every tensor lies in a GuardedBuffer whose payload ends at the back red zone; every channel outside a view's window - the pad channels
of the last 16-byte group among them, which the kernel loads - and every output start as the poison, a NaN.  After each launch the
result is free of poison, the channels outside the window (only coffset .. coffset + C - 1 may be written) still hold it bit for bit,
the inputs are unchanged and leaving the test checks every red zone.
Cases (tests/neuron_cases.py; tests/test_neuron_ref.py shows that each can fail): {1, 5, 49, 300} pixels x C in {6, 8, 10, 20, 68}, and
four odd widths at which the half kernel uses all three of its store forms - 16 bytes, 32-bit pairs, one half whose neighbour in the
same word is a poisoned pad half; ten configurations of the five modes; x a window at channel 4 of wider float pixels / 8 of wider half
pixels, y a buffer of its own or x itself; keep present with keep_cstride above round4(C); accumulate 0 and 1 into pre-filled
gradients; dx aliased to dy; every forward launched twice into fresh buffers: equal bytes; one launch per entry point whose grid-stride
loop takes a second trip.
float32 results: rel_err < 1e-4 against float64, the project's bound.  Half results, against float64 on the operands rounded to half:
per element within test_neuron_ref.half_allowance - 4 x the measured error of a float32 evaluation, half an ulp of the half, 2^-24."""
import numpy as np
import pytest

import neuron_cases as NC
import ref64
import ref_neuron64 as R
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched
from test_neuron_ref import half_allowance

pytestmark = pytest.mark.gpu
F32, F16 = np.float32, np.float16
TOL = 1e-4
E_ARG, E_ALIGN = 1, 2
MODE = {R.ELU: L.NEURON_ELU, R.CLIP: L.NEURON_CLIP, R.ABSVAL: L.NEURON_ABSVAL, R.BNLL: L.NEURON_BNLL, R.SWISH: L.NEURON_SWISH}
CASES = pytest.mark.parametrize("case", NC.CASES + NC.ODD_C, ids=NC.case_id)


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def ra(c, grp):
    return (c + grp - 1) // grp * grp


def windows(c, half):
    """(cstride, coffset) of x and of y: x at channel 4 of wider float pixels / 8 of wider half pixels, y at 0 of a stride of its own."""
    grp = 8 if half else 4
    return (grp + ra(c, grp) + (grp if half else 0), grp), (ra(c, grp) + grp, 0)


def check_f32(y, y64, what):
    err = R.rel_err(y, y64)
    print("REL %s %.3g" % (what, err))
    assert err < TOL, "%s: rel_err %.3g" % (what, err)


def check_f16(y, y64, allow, what):
    ratio, at = ref64.worst(y, y64, allow)
    print("BOUND %s %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (what, at, ratio)


def forward(g, case, half, configs, forms):
    p, c = case
    dt = F16 if half else F32
    x, _dy, _dx0 = NC.operands(case)
    if half:
        x = x.astype(F16)
    (xcs, xco), (ycs, yco) = windows(c, half)
    kcs = ra(c, 4) + 4
    for name, mode, a, b in configs:
        y64 = R.fwd(mode, x.astype(np.float64), F32(a), F32(b))      # (the parameters as the entry point receives them: floats)
        first = {}
        for form in forms:
            xd = g.put(poisoned_nhwc(x, xcs, xco, dtype=dt), at_end=True, name="x")
            yd, cs, co = (xd, xcs, xco) if form.startswith("y is x") else (g.put(poisoned((1, 1, p, ycs), dtype=dt), at_end=True, name="y"), ycs, yco)
            kd = g.put(poisoned((1, 1, p, kcs)), at_end=True, name="keep") if "keep" in form else None
            if half:
                L.call("fcn_neuron_fwd_f16", xd.ptr, yd.ptr, p, c, xcs, xco, cs, co, MODE[mode], a, b, None)
            else:
                L.call("fcn_neuron_fwd_f32", xd.ptr, yd.ptr, kd.ptr if kd is not None else None, p, c, xcs, xco, cs, co,
                       kcs if kd is not None else 0, MODE[mode], a, b, None)
            L.call("fcn_device_sync")
            full = yd.read((1, 1, p, cs), dt)
            y = nchw(full, c, co)
            what = "neuron_fwd_%s %s, %s p%d c%d" % ("f16" if half else "f32", name, form, p, c)
            assert poison_free(y), "%s: poison (a pad channel or a red zone) reached the result" % what
            if half:
                check_f16(y, y64, half_allowance(mode, y64), what)
            else:
                check_f32(y, y64, what)
            assert slice_untouched(full, co, c), "%s: channels of y outside the window were written" % what
            assert yd is xd or xd.unchanged(), "%s: an input was written" % what
            assert first.setdefault("y", y.tobytes()) == y.tobytes(), "%s: another launch on the same input gave other bytes" % what
            if kd is not None:
                kept = kd.read((1, 1, p, kcs))
                assert nchw(kept, c, 0).tobytes() == x.tobytes(), "%s: keep is not x, bit for bit" % what
                assert slice_untouched(kept, 0, c), "%s: channels of keep behind C were written" % what


def backward(g, case, configs, forms):
    p, c = case
    x, dy, dx0 = NC.operands(case)
    (dcs, dco), (xcs, xco) = windows(c, False)
    rcs = ra(c, 4) + 4                          # the reference operand as the kept copy lies: channels at 0 of a stride of its own
    for name, mode, a, b in configs:
        ref = R.ref_of(mode, x, F32(a), F32(b)).astype(F32)      # y as the forward launch stores it: a float32 blob
        for acc, alias in forms:
            dyd = g.put(poisoned_nhwc(dy, dcs, dco), at_end=True, name="dy")
            rd = g.put(poisoned_nhwc(ref, rcs, 0), at_end=True, name="ref")
            if alias:
                dxd, cs, co = dyd, dcs, dco
            else:
                dxd, cs, co = g.put(poisoned_nhwc(dx0, xcs, xco) if acc else poisoned((1, 1, p, xcs)), at_end=True, name="dx"), xcs, xco
            L.call("fcn_neuron_bwd_f32", dyd.ptr, rd.ptr, dxd.ptr, p, c, dcs, dco, rcs, 0, cs, co, MODE[mode], a, b, acc, None)
            L.call("fcn_device_sync")
            full = dxd.read((1, 1, p, cs))
            dx = nchw(full, c, co)
            what = "neuron_bwd %s acc%d%s p%d c%d" % (name, acc, " dx is dy" if alias else "", p, c)
            assert poison_free(dx), "%s: poison reached the result" % what
            check_f32(dx, R.bwd(mode, dy, ref, F32(a), F32(b), dx0 if acc else None), what)
            assert slice_untouched(full, co, c), "%s: channels of dx outside the window were written" % what
            assert (alias or dyd.unchanged()) and rd.unchanged(), "%s: an input was written" % what


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@CASES
def test_forward(g, case, half):
    forward(g, case, half, NC.CONFIGS, ("own y", "y is x", "own y again") + (() if half else ("own y, keep", "y is x, keep")))


@CASES
def test_data_gradient(g, case):
    backward(g, case, NC.CONFIGS, ((0, False), (1, False), (0, True)))


def test_a_second_trip_of_the_grid_stride_loop(g):
    """More pixels than the capped grid covers at once (tests/neuron_cases.py says where that is): the last ones belong to a second trip."""
    by_name = {cfg[0]: cfg for cfg in NC.CONFIGS}
    forward(g, NC.TRIP_F32, False, [by_name["swish beta -1.3"]], ("y is x, keep",))
    forward(g, NC.TRIP_F16, True, [by_name["elu alpha 0.7"]], ("own y",))
    backward(g, NC.TRIP_F32, [by_name["bnll"]], ((1, False),))


def test_refusals_by_error_code(g):
    lib = L.load()
    p, c = 5, 8
    xd = g.put(poisoned((p, 16)), name="x")
    yd = g.put(poisoned((p, 16)), name="y")
    kd = g.put(poisoned((p, 16)), name="keep")
    X, Y, K = xd.ptr, yd.ptr, kd.ptr
    EL, CL, AB, BN, SW = L.NEURON_ELU, L.NEURON_CLIP, L.NEURON_ABSVAL, L.NEURON_BNLL, L.NEURON_SWISH

    def f32(x=X, y=Y, keep=None, p=p, c=c, xcs=16, xco=0, ycs=16, yco=0, kcs=0, mode=SW, a=1.0, b=0.0):
        return lib.fcn_neuron_fwd_f32(x, y, keep, p, c, xcs, xco, ycs, yco, kcs, mode, a, b, None)

    def f16(x=X, y=Y, keep=None, p=p, c=c, xcs=16, xco=0, ycs=16, yco=0, kcs=0, mode=SW, a=1.0, b=0.0):
        return lib.fcn_neuron_fwd_f16(x, y, p, c, xcs, xco, ycs, yco, mode, a, b, None)

    def bd(x=X, ref=Y, y=K, keep=None, p=p, c=c, xcs=16, xco=0, rcs=16, rco=0, ycs=16, yco=0, mode=SW, a=1.0, b=0.0, acc=0):
        return lib.fcn_neuron_bwd_f32(x, ref, y, p, c, xcs, xco, rcs, rco, ycs, yco, mode, a, b, acc, None)

    for fn, grp in ((f32, 4), (f16, 8), (bd, 4)):
        assert fn(x=None) == E_ARG and fn(y=None) == E_ARG
        assert fn(p=0) == E_ARG and fn(c=0) == E_ARG and fn(mode=5) == E_ARG and fn(mode=-1) == E_ARG
        assert fn(mode=EL, a=-0.5) == E_ARG and fn(mode=EL, a=float("nan")) == E_ARG and fn(mode=EL, a=0.0) == 0
        assert fn(mode=CL, a=6.0, b=6.0) == E_ARG and fn(mode=CL, a=1.0, b=0.0) == E_ARG and fn(mode=CL, a=0.0, b=float("nan")) == E_ARG
        assert fn(mode=CL, a=-2.0, b=-1.0) == 0
        assert fn(xco=16) == E_ARG and fn(yco=-grp) == E_ARG and fn(ycs=4) == E_ARG      # the window leaves the pixel
        assert fn(xcs=16 + grp // 2) == E_ALIGN and fn(xcs=32, xco=grp // 2) == E_ALIGN and fn(ycs=32, yco=grp // 2) == E_ALIGN
        assert fn(x=X + 8) == E_ALIGN and fn(y=Y + 4) == E_ALIGN
        assert all(fn(mode=m, a=-1.0, b=-2.0) == 0 for m in (AB, BN, SW))      # a and b are ignored where the mode has no use for them
        assert fn() == 0
    assert f16(xcs=12, xco=4, c=4) == E_ALIGN                      # (a window at 4 of 12 is a float32 window: halves come in groups of 8)
    assert f32(keep=K, kcs=4) == E_ARG and f32(keep=K, kcs=10) == E_ALIGN and f32(keep=K + 8, kcs=16) == E_ALIGN and f32(keep=K, kcs=16) == 0
    assert bd(ref=None) == E_ARG and bd(rco=12) == E_ARG and bd(rcs=4) == E_ARG and bd(rcs=18) == E_ALIGN and bd(ref=Y + 8) == E_ALIGN
    assert bd(y=X) == 0 and bd(acc=1) == 0 and f32(y=X) == 0 and f16(y=X) == 0      # dx may be dy, y may be x
    L.call("fcn_device_sync")
