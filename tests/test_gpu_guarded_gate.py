"""The gated-Scale entry points (csrc/gate.hip) in guard-banded, poisoned buffers against tests/ref_gate64.py, -m gpu.

Every tensor lies in a GuardedBuffer whose payload ends at the back red zone; every channel outside a view's window, the floats of a
gate row behind its C values and every output start as the poison.  After each launch the result is free of poison, the channels
outside the window (the pad channels of y / dx: only coffset .. coffset + C - 1 may be written) and the gate rows' tails still hold it
bit for bit, the inputs are unchanged and leaving the test checks every red zone.
Cases (tests/gate_cases.py, which also says which of them cross the slab boundary of the gate gradient - 300 pixels at every C, 49 at
C = 20 and 68 - and tests/test_gate_ref.py shows that each can fail): N = 2, 3; 1, 5, 49, 300 pixels per image; C = 6, 8, 20, 68, and in the half-float forward (N = 2) the odd C = 3, 5, 7, 13; x a
window at channel 4 of 12-float pixels / 8 of 24-half pixels (wider where C needs it); g_rstride = C + 3; r absent or present with a
stride of its own; y a buffer of its own, x, or r; relu on and off; accumulate 0 and 1 into pre-filled gradients.
float32 results: rel_err < 1e-4 against float64, the project's bound.  Half results: against float64 on the operands rounded to half,
within half an ulp of the rounded result (U16 |y|, the bound of tests/test_gpu_guarded_tconv_f16.py) plus the two float32 roundings
of the product and the sum on their magnitudes.  The gate gradient runs twice into fresh buffers: equal bytes."""
import numpy as np
import pytest

import gate_cases as GC
import ref64
import ref_gate64 as R
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu
F32, F16 = np.float32, np.float16
TOL = 1e-4
E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def ra(c, grp):
    return (c + grp - 1) // grp * grp


def windows(c, half):
    """(cstride, coffset) of x, of r and of y: x at channel 4 of 12 floats / 8 of 24 halves where C fits, r and y with strides of their own."""
    grp = 8 if half else 4
    return (grp + ra(c, grp) + (grp if half else 0), grp), (ra(c, grp) + 2 * grp, grp), (ra(c, grp) + grp, 0)


def gate_rows(g, gate, grs, name="gate"):
    n, c = gate.shape
    rows = poisoned((n, grs))
    rows[:, :c] = gate
    return g.put(rows.reshape(-1)[:(n - 1) * grs + c], at_end=True, name=name)      # the last row ends with its C values


def check_f32(y, y64, what):
    err = R.rel_err(y, y64)
    print("REL %s %.3g" % (what, err))
    assert err < TOL, "%s: rel_err %.3g" % (what, err)


def check_f16(y, y64, mag, what):
    allow = 2 * ref64.U32 * mag + ref64.U16 * np.abs(y64) + 2.0 ** -24
    ratio, at = ref64.worst(y, y64, allow)
    print("BOUND %s %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (what, at, ratio)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", GC.SHAPES, ids=lambda s: "n%d_%dx%d_c%d" % s)
def test_forward(g, shape, half):
    n, h, w, c = shape
    dt = F16 if half else F32
    x, gate, r, _dy, _dx0, _dg0 = GC.operands(shape)
    if half:
        x, r = x.astype(F16), r.astype(F16)
    x64, r64, g64 = x.astype(np.float64), r.astype(np.float64), gate.astype(np.float64)
    (xcs, xco), (rcs, rco), (ycs, yco) = windows(c, half)
    grs = c + 3
    fn = "fcn_scale_gate_fwd_f16" if half else "fcn_scale_gate_fwd_f32"
    for mode in ("plain", "residual", "y is x", "y is r"):
        for relu in (0, 1):
            xd = g.put(poisoned_nhwc(x, xcs, xco, dtype=dt), at_end=True, name="x")
            gd = gate_rows(g, gate, grs)
            rd = g.put(poisoned_nhwc(r, rcs, rco, dtype=dt), at_end=True, name="r") if mode != "plain" else None
            own = g.put(poisoned((n, h, w, ycs), dtype=dt), at_end=True, name="y") if mode in ("plain", "residual") else None
            yd, cs, co = {"plain": (own, ycs, yco), "residual": (own, ycs, yco), "y is x": (xd, xcs, xco), "y is r": (rd, rcs, rco)}[mode]
            with_r = mode != "plain"
            L.call(fn, xd.ptr, gd.ptr, rd.ptr if with_r else None, yd.ptr, n, h * w, c, xcs, xco, grs, rcs if with_r else 0, rco if with_r else 0,
                   cs, co, relu, None)
            L.call("fcn_device_sync")
            full = yd.read((n, h, w, cs), dt)
            y = nchw(full, c, co)
            what = "%s %s relu%d n%d p%d c%d" % (fn, mode, relu, n, h * w, c)
            assert poison_free(y), "%s: poison (a pad channel, the tail of a gate row or a red zone) reached the result" % what
            y64 = R.gate_fwd(x64, g64, r64 if with_r else None, bool(relu))
            if half:
                check_f16(y, y64, np.abs(x64 * g64[:, :, None, None]) + (np.abs(r64) if with_r else 0.0), what)
            else:
                check_f32(y, y64, what)
            assert slice_untouched(full, co, c), "%s: channels of y outside the window were written" % what
            assert gd.unchanged() and (yd is xd or xd.unchanged()) and (rd is None or yd is rd or rd.unchanged()), "%s: an input was written" % what


@pytest.mark.parametrize("shape", GC.ODD_SHAPES, ids=lambda s: "n%d_%dx%d_c%d" % s)
def test_forward_half_floats_at_odd_widths(g, shape):
    """The last half of a window shares its 32-bit word with a pad channel: every mode of test_forward, without and with the residual."""
    assert shape[0] == 2 and shape[3] % 2 == 1
    test_forward(g, shape, True)


@pytest.mark.parametrize("shape", GC.SHAPES, ids=lambda s: "n%d_%dx%d_c%d" % s)
def test_data_gradient(g, shape):
    n, h, w, c = shape
    _x, gate, _r, dy, dx0, _dg0 = GC.operands(shape)
    (dcs, dco), (xcs, xco), _ = windows(c, False)
    grs = c + 3
    for acc in (0, 1):
        dyd = g.put(poisoned_nhwc(dy, dcs, dco), at_end=True, name="dy")
        gd = gate_rows(g, gate, grs)
        dxd = g.put(poisoned_nhwc(dx0, xcs, xco) if acc else poisoned((n, h, w, xcs)), at_end=True, name="dx")
        L.call("fcn_scale_gate_bwd_data_f32", dyd.ptr, gd.ptr, dxd.ptr, n, h * w, c, dcs, dco, grs, xcs, xco, acc, None)
        L.call("fcn_device_sync")
        full = dxd.read((n, h, w, xcs))
        dx = nchw(full, c, xco)
        what = "scale_gate_bwd_data acc%d n%d p%d c%d" % (acc, n, h * w, c)
        assert poison_free(dx), "%s: poison reached the result" % what
        check_f32(dx, R.gate_bwd_data(dy, gate, dx0 if acc else None), what)
        assert slice_untouched(full, xco, c) and dyd.unchanged() and gd.unchanged(), what
    # dx may be dy
    dyd = g.put(poisoned_nhwc(dy, dcs, dco), at_end=True, name="dy = dx")
    gd = gate_rows(g, gate, grs)
    L.call("fcn_scale_gate_bwd_data_f32", dyd.ptr, gd.ptr, dyd.ptr, n, h * w, c, dcs, dco, grs, dcs, dco, 0, None)
    L.call("fcn_device_sync")
    full = dyd.read((n, h, w, dcs))
    check_f32(nchw(full, c, dco), R.gate_bwd_data(dy, gate), "scale_gate_bwd_data in place n%d p%d c%d" % (n, h * w, c))
    assert slice_untouched(full, dco, c)


@pytest.mark.parametrize("shape", GC.SHAPES, ids=lambda s: "n%d_%dx%d_c%d" % s)
def test_gate_gradient(g, shape):
    n, h, w, c = shape
    x, _gate, _r, dy, _dx0, dg0 = GC.operands(shape)
    (xcs, xco), (dcs, dco), _ = windows(c, False)
    grs = c + 3
    nbytes = int(L.load().fcn_scale_gate_workspace_bytes(n, h * w, c))
    slabs = -(-h * w // GC.first_slab(c))
    assert nbytes == n * slabs * ra(c, 4) * 4 and (slabs > 1) == GC.crosses_a_slab(shape)
    dyd = g.put(poisoned_nhwc(dy, dcs, dco), at_end=True, name="dy")
    xd = g.put(poisoned_nhwc(x, xcs, xco), at_end=True, name="x")
    for acc in (0, 1):
        outs = []
        for rep in range(2):
            ws = g.put(nbytes, name="workspace run %d" % rep)
            rows = poisoned((n, grs))
            if acc:
                rows[:, :c] = dg0
            dgd = g.put(rows.reshape(-1)[:(n - 1) * grs + c], at_end=True, name="dgate run %d" % rep)
            L.call("fcn_scale_gate_bwd_gate_f32", dyd.ptr, xd.ptr, dgd.ptr, n, h * w, c, dcs, dco, xcs, xco, grs, acc, ws.ptr, None)
            L.call("fcn_device_sync")
            flat = np.concatenate([dgd.read(((n - 1) * grs + c,)), poisoned((grs - c,))])
            outs.append(flat.reshape(n, grs))
        assert outs[0].tobytes() == outs[1].tobytes(), "two identical calls gave different bytes"
        what = "scale_gate_bwd_gate acc%d n%d p%d c%d (%d slabs)" % (acc, n, h * w, c, slabs)
        dg = outs[0][:, :c]
        assert poison_free(dg), "%s: poison reached the result" % what
        check_f32(dg, R.gate_bwd_gate(dy, x, dg0 if acc else None), what)
        assert slice_untouched(outs[0], 0, c), "%s: floats behind a row's C values were written" % what
        assert dyd.unchanged() and xd.unchanged(), what


def test_refusals_by_error_code(g):
    lib = L.load()
    n, p, c = 2, 5, 8
    xd = g.put(poisoned((n, p, 16)), name="x")
    yd = g.put(poisoned((n, p, 16)), name="y")
    gd = g.put(poisoned((n, 12)), name="gate")
    ws = g.put(max(int(lib.fcn_scale_gate_workspace_bytes(n, p, c)), 16), name="workspace")
    X, Y, G, W = xd.ptr, yd.ptr, gd.ptr, ws.ptr

    def fwd(fn=lib.fcn_scale_gate_fwd_f32, x=X, gate=G, r=None, y=Y, n=n, p=p, c=c, xcs=16, xco=0, grs=12, rcs=0, rco=0, ycs=16, yco=0):
        return fn(x, gate, r, y, n, p, c, xcs, xco, grs, rcs, rco, ycs, yco, 0, None)

    for fn, grp in ((lib.fcn_scale_gate_fwd_f32, 4), (lib.fcn_scale_gate_fwd_f16, 8)):
        assert fwd(fn, x=None) == E_ARG and fwd(fn, gate=None) == E_ARG and fwd(fn, y=None) == E_ARG
        assert fwd(fn, n=0) == E_ARG and fwd(fn, p=0) == E_ARG and fwd(fn, c=0) == E_ARG
        assert fwd(fn, xco=16) == E_ARG and fwd(fn, yco=-grp) == E_ARG and fwd(fn, ycs=4) == E_ARG      # the window leaves the pixel
        assert fwd(fn, r=X, rcs=4, rco=0) == E_ARG and fwd(fn, grs=c - 1) == E_ARG
        assert fwd(fn, xcs=16 + grp // 2, xco=0) == E_ALIGN and fwd(fn, xcs=32, xco=grp // 2) == E_ALIGN and fwd(fn, r=X, rcs=18, rco=2) == E_ALIGN
        assert fwd(fn, x=X + 8) == E_ALIGN and fwd(fn, y=Y + 4) == E_ALIGN and fwd(fn, r=X + 8, rcs=16) == E_ALIGN and fwd(fn, gate=G + 2) == E_ALIGN
        assert fwd(fn, n=65536) == E_UNSUPPORTED and fwd(fn, n=4096, p=1 << 19) == E_UNSUPPORTED
        assert fwd(fn) == 0
    bd = lambda dy=X, gate=G, dx=Y, n=n, c=c, dcs=16, dco=0, grs=12, xcs=16, xco=0, acc=0: lib.fcn_scale_gate_bwd_data_f32(
        dy, gate, dx, n, p, c, dcs, dco, grs, xcs, xco, acc, None)
    assert bd(dy=None) == E_ARG and bd(gate=None) == E_ARG and bd(dx=None) == E_ARG and bd(c=0) == E_ARG and bd(xco=12) == E_ARG and bd(grs=7) == E_ARG
    assert bd(dcs=18) == E_ALIGN and bd(xco=2, xcs=32) == E_ALIGN and bd(dx=Y + 4) == E_ALIGN and bd(n=65536) == E_UNSUPPORTED and bd() == 0
    bg = lambda dy=X, x=Y, dg=G, n=n, c=c, dcs=16, dco=0, xcs=16, xco=0, grs=12, w=W: lib.fcn_scale_gate_bwd_gate_f32(
        dy, x, dg, n, p, c, dcs, dco, xcs, xco, grs, 0, w, None)
    assert bg(dy=None) == E_ARG and bg(x=None) == E_ARG and bg(dg=None) == E_ARG and bg(w=None) == E_ARG and bg(c=-1) == E_ARG
    assert bg(dco=12) == E_ARG and bg(grs=7) == E_ARG
    assert bg(xcs=18) == E_ALIGN and bg(dco=2, dcs=32) == E_ALIGN and bg(x=Y + 8) == E_ALIGN and bg(w=W + 4) == E_ALIGN and bg(dg=G + 1) == E_ALIGN
    assert bg(n=65536) == E_UNSUPPORTED
    assert lib.fcn_scale_gate_workspace_bytes(0, p, c) == 0 and lib.fcn_scale_gate_workspace_bytes(n, p, 0) == 0
    L.call("fcn_device_sync")
