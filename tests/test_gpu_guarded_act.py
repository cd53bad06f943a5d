"""The activation entry points (csrc/act.hip: PReLU, TanH, Bias) in guard-banded, poisoned buffers against tests/ref_act64.py, -m gpu.

Every tensor lies in a GuardedBuffer whose payload ends at the back red zone; every channel outside a view's window and every output
start as the poison; the parameters end at the red zone too (a shared slope is ONE float: a lane that reads param[c] reads poison).
After each launch the result is free of poison, the channels outside the window (only coffset .. coffset + C - 1 may be written) still
hold it bit for bit, the inputs are unchanged and leaving the test checks every red zone.
Cases (tests/act_cases.py, which says where the slab boundaries of the parameter gradient lie; tests/test_act_ref.py shows that each
case can fail): 1, 5, 49, 300 pixels, one count on each side of the slab boundary at C = 6, 10, 20, 68 and two counts of more than 64
slabs; C = 6, 8, 10, 20, 68, and in the half-float forward the odd C = 3, 5, 7, 13; x a window at channel 4 of wider float pixels / 8 of wider half pixels, y a buffer of its own or x itself;
keep present with keep_cstride above round4(C); the slopes per channel (both signs and zero) and shared (negative); accumulate 0 and 1
into pre-filled gradients; dx aliased to dy.
float32 results: rel_err < 1e-4 against float64, the project's bound.  Half results, against float64 on the operands rounded to half:
PReLU and Bias within U32 * mag + U16 |y| + 2^-24 (one float32 rounding, half an ulp for the store), TanH within one ulp of the half,
2 U16 |y| + 2^-24 (tests/test_act_ref.py derives both and shows that they admit a float32 evaluation).  The parameter gradient runs
twice into fresh buffers: equal bytes."""
import numpy as np
import pytest

import act_cases as AC
import ref64
import ref_act64 as R
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched
from test_act_ref import half_allowance, half_magnitude

pytestmark = pytest.mark.gpu
F32, F16 = np.float32, np.float16
TOL = 1e-4
E_ARG, E_ALIGN = 1, 2
CASES = pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)
SHARED = np.array([AC.SHARED_SLOPE], F32)


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


def modes(a, b):
    """(name, mode, parameter or None, shared)"""
    return (("prelu", L.ACT_PRELU, a, 0), ("prelu shared", L.ACT_PRELU, SHARED, 1), ("tanh", L.ACT_TANH, None, 0), ("bias", L.ACT_BIAS, b, 0))


def ref_mode(mode):
    return {L.ACT_PRELU: R.PRELU, L.ACT_TANH: R.TANH, L.ACT_BIAS: R.BIAS}[mode]


def check_f32(y, y64, what):
    err = R.rel_err(y, y64)
    print("REL %s %.3g" % (what, err))
    assert err < TOL, "%s: rel_err %.3g" % (what, err)


def check_f16(y, y64, allow, what):
    ratio, at = ref64.worst(y, y64, allow)
    print("BOUND %s %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (what, at, ratio)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@CASES
def test_forward(g, case, half):
    p, c = case
    dt = F16 if half else F32
    x, a, b, _dy, _dx0 = AC.operands(case)
    if half:
        x = x.astype(F16)
    x64 = x.astype(np.float64)
    (xcs, xco), (ycs, yco) = windows(c, half)
    kcs = ra(c, 4) + 4
    for name, mode, par, shared in modes(a, b):
        y64 = R.fwd(ref_mode(mode), x64, par, bool(shared))
        for form in ("own y", "y is x") + (() if half else ("own y, keep", "y is x, keep")):
            xd = g.put(poisoned_nhwc(x, xcs, xco, dtype=dt), at_end=True, name="x")
            pd = g.put(par, at_end=True, name="param") if par is not None else None
            yd, cs, co = (xd, xcs, xco) if form.startswith("y is x") else (g.put(poisoned((1, 1, p, ycs), dtype=dt), at_end=True, name="y"), ycs, yco)
            kd = g.put(poisoned((1, 1, p, kcs)), at_end=True, name="keep") if "keep" in form else None
            pp = pd.ptr if pd is not None else None
            if half:
                L.call("fcn_act_fwd_f16", xd.ptr, yd.ptr, p, c, xcs, xco, cs, co, mode, pp, shared, None)
            else:
                L.call("fcn_act_fwd_f32", xd.ptr, yd.ptr, kd.ptr if kd is not None else None, p, c, xcs, xco, cs, co, kcs if kd is not None else 0,
                       mode, pp, shared, None)
            L.call("fcn_device_sync")
            full = yd.read((1, 1, p, cs), dt)
            y = nchw(full, c, co)
            what = "act_fwd_%s %s, %s p%d c%d" % ("f16" if half else "f32", name, form, p, c)
            assert poison_free(y), "%s: poison (a pad channel, the float behind a shared slope or a red zone) reached the result" % what
            if half:
                check_f16(y, y64, half_allowance(ref_mode(mode), y64, half_magnitude(ref_mode(mode), x64, None if par is None else par.astype(np.float64),
                                                                                     bool(shared))), what)
            else:
                check_f32(y, y64, what)
            assert slice_untouched(full, co, c), "%s: channels of y outside the window were written" % what
            assert (yd is xd or xd.unchanged()) and (pd is None or pd.unchanged()), "%s: an input was written" % what
            if kd is not None:
                kept = kd.read((1, 1, p, kcs))
                assert nchw(kept, c, 0).tobytes() == x.tobytes(), "%s: keep is not x, bit for bit" % what
                assert slice_untouched(kept, 0, c), "%s: channels of keep behind C were written" % what


@pytest.mark.parametrize("case", AC.ODD_C, ids=AC.case_id)
def test_forward_half_floats_at_odd_widths(g, case):
    """The last half of a window shares its 32-bit word with a pad channel: every mode and form of test_forward, x a window at channel 8."""
    assert case[1] % 2 == 1 and windows(case[1], True)[0][1] == 8
    test_forward(g, case, True)


@CASES
def test_data_gradient(g, case):
    p, c = case
    x, a, b, dy, dx0 = AC.operands(case)
    (dcs, dco), (xcs, xco) = windows(c, False)
    rcs = ra(c, 4) + 4                          # the reference operand as the kept copy lies: channels at 0 of a stride of its own
    for name, mode, par, shared in modes(a, b):
        rm = ref_mode(mode)
        ref = x if mode == L.ACT_PRELU else R.fwd(R.TANH, x).astype(F32) if mode == L.ACT_TANH else None
        for acc, alias in ((0, False), (1, False), (0, True)):
            dyd = g.put(poisoned_nhwc(dy, dcs, dco), at_end=True, name="dy")
            rd = g.put(poisoned_nhwc(ref, rcs, 0), at_end=True, name="ref") if ref is not None else None
            pd = g.put(par, at_end=True, name="param") if mode == L.ACT_PRELU else None
            if alias:
                dxd, cs, co = dyd, dcs, dco
            else:
                dxd, cs, co = g.put(poisoned_nhwc(dx0, xcs, xco) if acc else poisoned((1, 1, p, xcs)), at_end=True, name="dx"), xcs, xco
            L.call("fcn_act_bwd_data_f32", dyd.ptr, rd.ptr if rd is not None else None, dxd.ptr, p, c, dcs, dco, rcs if rd is not None else 0, 0,
                   cs, co, mode, pd.ptr if pd is not None else None, shared, acc, None)
            L.call("fcn_device_sync")
            full = dxd.read((1, 1, p, cs))
            dx = nchw(full, c, co)
            what = "act_bwd_data %s acc%d%s p%d c%d" % (name, acc, " dx is dy" if alias else "", p, c)
            assert poison_free(dx), "%s: poison reached the result" % what
            check_f32(dx, R.bwd_data(rm, dy, ref, par, bool(shared), dx0 if acc else None), what)
            assert slice_untouched(full, co, c), "%s: channels of dx outside the window were written" % what
            assert (alias or dyd.unchanged()) and (rd is None or rd.unchanged()) and (pd is None or pd.unchanged()), "%s: an input was written" % what


@CASES
def test_parameter_gradient(g, case):
    p, c = case
    x, _a, _b, dy, _dx0 = AC.operands(case)
    (dcs, dco), (xcs, xco) = windows(c, False)
    nbytes = int(L.load().fcn_act_workspace_bytes(p, c))
    assert nbytes == AC.workspace_bytes(case), (nbytes, AC.workspace_bytes(case))
    dyd = g.put(poisoned_nhwc(dy, dcs, dco), at_end=True, name="dy")
    xd = g.put(poisoned_nhwc(x, xcs, xco), at_end=True, name="x")
    for mode in (L.ACT_PRELU, L.ACT_BIAS):
        for shared in (0, 1):
            outs = []
            for rep in range(2):
                ws = g.put(nbytes, name="workspace run %d" % rep)
                dpd = g.put(poisoned((1 if shared else c,)), at_end=True, name="dparam run %d" % rep)      # poison: the result is overwritten
                L.call("fcn_act_bwd_param_f32", dyd.ptr, xd.ptr if mode == L.ACT_PRELU else None, dpd.ptr, p, c, dcs, dco, xcs, xco, mode, shared,
                       ws.ptr, None)
                L.call("fcn_device_sync")
                outs.append(dpd.read((1 if shared else c,)))
            assert outs[0].tobytes() == outs[1].tobytes(), "two identical calls gave different bytes"
            what = "act_bwd_param %s%s p%d c%d (%d slabs)" % (ref_mode(mode), " shared" if shared else "", p, c, AC.slabs(case))
            assert poison_free(outs[0]), "%s: poison reached the result" % what
            check_f32(outs[0], R.bwd_param(ref_mode(mode), dy, x, bool(shared)), what)
            assert dyd.unchanged() and xd.unchanged(), what


def test_refusals_by_error_code(g):
    lib = L.load()
    p, c = 5, 8
    xd = g.put(poisoned((p, 16)), name="x")
    yd = g.put(poisoned((p, 16)), name="y")
    kd = g.put(poisoned((p, 16)), name="keep")
    pd = g.put(poisoned((c,)), name="param")
    ws = g.put(max(int(lib.fcn_act_workspace_bytes(p, c)), 16), name="workspace")
    X, Y, K, P, W = xd.ptr, yd.ptr, kd.ptr, pd.ptr, ws.ptr
    PR, TH, BI = L.ACT_PRELU, L.ACT_TANH, L.ACT_BIAS

    def f32(x=X, y=Y, keep=None, p=p, c=c, xcs=16, xco=0, ycs=16, yco=0, kcs=0, mode=PR, par=P, shared=0):
        return lib.fcn_act_fwd_f32(x, y, keep, p, c, xcs, xco, ycs, yco, kcs, mode, par, shared, None)

    def f16(x=X, y=Y, keep=None, p=p, c=c, xcs=16, xco=0, ycs=16, yco=0, kcs=0, mode=PR, par=P, shared=0):
        return lib.fcn_act_fwd_f16(x, y, p, c, xcs, xco, ycs, yco, mode, par, shared, None)

    for fn, grp in ((f32, 4), (f16, 8)):
        assert fn(x=None) == E_ARG and fn(y=None) == E_ARG and fn(par=None) == E_ARG and fn(par=None, mode=BI) == E_ARG
        assert fn(p=0) == E_ARG and fn(c=0) == E_ARG and fn(mode=3) == E_ARG and fn(mode=-1) == E_ARG
        assert fn(xco=16) == E_ARG and fn(yco=-grp) == E_ARG and fn(ycs=4) == E_ARG      # the window leaves the pixel
        assert fn(xcs=16 + grp // 2) == E_ALIGN and fn(xcs=32, xco=grp // 2) == E_ALIGN and fn(ycs=32, yco=grp // 2) == E_ALIGN
        assert fn(x=X + 8) == E_ALIGN and fn(y=Y + 4) == E_ALIGN and fn(par=P + 2) == E_ALIGN
        assert fn(par=None, mode=TH) == 0 and fn() == 0
    assert f16(xcs=12, xco=4, c=4) == E_ALIGN                      # (a window at 4 of 12 is a float32 window: halves come in groups of 8)
    assert f32(keep=K, kcs=4) == E_ARG and f32(keep=K, kcs=10) == E_ALIGN and f32(keep=K + 8, kcs=16) == E_ALIGN and f32(keep=K, kcs=16) == 0

    def bd(dy=X, ref=Y, dx=K, c=c, dcs=16, dco=0, rcs=16, rco=0, xcs=16, xco=0, mode=PR, par=P, acc=0):
        return lib.fcn_act_bwd_data_f32(dy, ref, dx, p, c, dcs, dco, rcs, rco, xcs, xco, mode, par, 0, acc, None)
    assert bd(dy=None) == E_ARG and bd(dx=None) == E_ARG and bd(ref=None) == E_ARG and bd(ref=None, mode=TH) == E_ARG and bd(par=None) == E_ARG
    assert bd(c=0) == E_ARG and bd(mode=7) == E_ARG and bd(xco=12) == E_ARG and bd(rcs=4) == E_ARG
    assert bd(dcs=18) == E_ALIGN and bd(xco=2, xcs=32) == E_ALIGN and bd(rcs=18) == E_ALIGN and bd(dx=K + 4) == E_ALIGN and bd(ref=Y + 8) == E_ALIGN
    assert bd(ref=None, par=None, mode=BI, rcs=3, rco=-1) == 0 and bd(par=None, mode=TH) == 0 and bd() == 0 and bd(dx=X) == 0

    def bp(dy=X, x=Y, dp=P, c=c, dcs=16, dco=0, xcs=16, xco=0, mode=PR, shared=0, w=W):
        return lib.fcn_act_bwd_param_f32(dy, x, dp, p, c, dcs, dco, xcs, xco, mode, shared, w, None)
    assert bp(mode=TH) == E_ARG and b"no parameter" in lib.fcn_last_error_string()
    assert bp(dy=None) == E_ARG and bp(x=None) == E_ARG and bp(dp=None) == E_ARG and bp(w=None) == E_ARG and bp(c=-1) == E_ARG and bp(dco=12) == E_ARG
    assert bp(xcs=18) == E_ALIGN and bp(dco=2, dcs=32) == E_ALIGN and bp(x=Y + 8) == E_ALIGN and bp(w=W + 4) == E_ALIGN and bp(dp=P + 1) == E_ALIGN
    assert bp(x=None, mode=BI, xcs=3) == 0 and bp() == 0 and bp(shared=1) == 0
    assert lib.fcn_act_workspace_bytes(0, c) == 0 and lib.fcn_act_workspace_bytes(p, 0) == 0 and lib.fcn_act_workspace_bytes(p, c) == 2 * 8 * 4
    L.call("fcn_device_sync")
