"""The entry points of csrc/shuffle.hip (ShuffleChannel, forward and - with group C / g - its data gradient) in guard-banded, poisoned
buffers against tests/ref_shuffle64.py, -m gpu.

Every tensor lies in a GuardedBuffer whose payload ends at the back red zone; every channel outside a view's window - the pad channels
of x among them, which hold NaN - and every output start as the poison.  After each launch the result is free of poison and equals the
reference BIT FOR BIT in both element types (the kernel moves values; the accumulate's one add has exact operands), the channels outside
y's window still hold the poison, x is unchanged and leaving the test checks every red zone.
Cases (tests/shuffle_cases.py; tests/test_shuffle_ref.py shows that each can fail): the (C, g) pairs there in both element types, at
1 pixel and at one less and one more than a workgroup's rows; x and y as whole buffers and as windows at channel 4 (8 in halves) of
wider pixels; accumulate 0 and 1 onto a pre-filled y; every launch repeated into fresh buffers: equal bytes; one launch per entry point
whose grid-stride loop takes a second trip; every refusal by its code, with nothing written."""
import numpy as np
import pytest

import ref_shuffle64 as R
import shuffle_cases as SC
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu
F32, F16 = np.float32, np.float16
E_ARG, E_ALIGN = 1, 2
CASES = pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
HALF = pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def ra(c, grp):
    return (c + grp - 1) // grp * grp


def windows(c, grp, form):
    """(cstride, coffset) of x and of y: whole buffers, or windows at channel `grp` of wider pixels with pad channels on both sides."""
    if form == "whole":
        return (ra(c, grp), 0), (ra(c, grp), 0)
    return (grp + ra(c, grp) + grp, grp), (grp + ra(c, grp) + 2 * grp, grp)


def launch(g, p, c, group, half, form, acc, first):
    dt, grp = (F16, 8) if half else (F32, 4)
    x, y0 = SC.operands(p, c, dt)
    (xcs, xco), (ycs, yco) = windows(c, grp, form)
    xd = g.put(poisoned_nhwc(x, xcs, xco, dtype=dt), at_end=True, name="x")
    yd = g.put(poisoned_nhwc(y0, ycs, yco, dtype=dt) if acc else poisoned((1, 1, p, ycs), dtype=dt), at_end=True, name="y")
    if half:
        L.call("fcn_shuffle_channel_f16", xd.ptr, yd.ptr, p, c, group, xcs, xco, ycs, yco, None)
    else:
        L.call("fcn_shuffle_channel_f32", xd.ptr, yd.ptr, p, c, group, xcs, xco, ycs, yco, acc, None)
    L.call("fcn_device_sync")
    full = yd.read((1, 1, p, ycs), dt)
    y = nchw(full, c, yco)
    what = "shuffle_channel_%s c%d g%d p%d %s acc%d" % ("f16" if half else "f32", c, group, p, form, acc)
    want = R.fwd(x, group)
    if acc:
        want = (y0 + want).astype(dt)
    assert poison_free(y), "%s: poison (a pad channel or a red zone) reached the result" % what
    print("MISMATCH %s %d of %d" % (what, int(np.count_nonzero(y != want)), y.size))
    assert y.tobytes() == want.tobytes(), "%s: not the reference, bit for bit" % what
    assert slice_untouched(full, yco, c), "%s: channels of y outside the window were written" % what
    assert xd.unchanged(), "%s: x was written" % what
    assert first.setdefault((form, acc), y.tobytes()) == y.tobytes(), "%s: another launch on the same input gave other bytes" % what
    return y, x


@HALF
@CASES
def test_forward(g, case, half):
    c, group = case
    for p in SC.pixel_counts(c, 8 if half else 4):
        first = {}
        for form in ("whole", "windows", "windows"):
            y, x = launch(g, p, c, group, half, form, 0, first)
            if case in SC.IDENTITY:
                assert y.tobytes() == x.tobytes()
            else:
                assert y.tobytes() != x.tobytes()


@CASES
def test_the_gradient_is_the_launch_with_group_c_over_g_and_accumulates(g, case):
    """What backward._shuffle launches: group C / g, accumulate 0 into a poisoned dx and 1 onto a pre-filled one."""
    c, group = case
    for p in SC.pixel_counts(c, 4):
        x, y0 = SC.operands(p, c)
        first = {}
        for form in ("whole", "windows"):
            for acc in (0, 1, 1):
                dx, dy = launch(g, p, c, c // group, False, form, acc, first)
                assert dx.tobytes() == R.bwd(dy, group, y0 if acc else None).tobytes()
        if case not in SC.IDENTITY:
            assert first[("whole", 1)] != first[("whole", 0)]


def test_a_second_trip_of_the_grid_stride_loop(g):
    """More pixels than the capped grid covers at once (tests/shuffle_cases.py says where that is): the last ones belong to a second trip."""
    p, c, group = SC.TRIP_F32
    launch(g, p, c, group, False, "windows", 1, {})
    p, c, group = SC.TRIP_F16
    launch(g, p, c, group, True, "windows", 0, {})


def test_refusals_by_error_code(g):
    lib = L.load()
    p, c = 5, 12
    xd = g.put(poisoned((p, 32)), name="x")
    yd = g.put(poisoned((p, 32)), name="y")
    X, Y = xd.ptr, yd.ptr

    def f32(x=X, y=Y, p=p, c=c, grp=3, xcs=16, xco=0, ycs=16, yco=0, acc=0):
        return lib.fcn_shuffle_channel_f32(x, y, p, c, grp, xcs, xco, ycs, yco, acc, None)

    def f16(x=X, y=Y, p=p, c=c, grp=3, xcs=16, xco=0, ycs=16, yco=0, acc=0):
        return lib.fcn_shuffle_channel_f16(x, y, p, c, grp, xcs, xco, ycs, yco, None)

    for fn, grp in ((f32, 4), (f16, 8)):
        assert fn(x=None) == E_ARG and fn(y=None) == E_ARG and fn(p=0) == E_ARG and fn(c=0) == E_ARG
        assert fn(grp=0) == E_ARG and fn(grp=-1) == E_ARG and fn(grp=5) == E_ARG and fn(grp=8) == E_ARG      # C % group != 0
        assert fn(xco=16) == E_ARG and fn(yco=-grp) == E_ARG and fn(ycs=8) == E_ARG                           # the window leaves the pixel
        assert fn(xcs=16 + grp // 2) == E_ALIGN and fn(xcs=32, xco=grp // 2) == E_ALIGN and fn(ycs=32, yco=grp // 2) == E_ALIGN
        assert fn(x=X + 8) == E_ALIGN and fn(y=Y + 4) == E_ALIGN
        # overlapping windows: in place, y starting inside x's bytes, and two windows of one buffer interleaved pixel by pixel
        assert fn(y=X) == E_ARG and fn(y=X + 64) == E_ARG and fn(x=Y + 32, p=3) == E_ARG
        assert fn(y=X, xcs=32, ycs=32, yco=16, p=2) == E_ARG
    assert f16(xcs=12, xco=4, c=4, grp=2) == E_ALIGN      # (a window at 4 of 12 is a float32 window: halves come in groups of 8)
    L.call("fcn_device_sync")
    assert xd.unchanged() and yd.unchanged(), "a refused call wrote"
    for fn in (f32, f16):      # (and what is not refused: the identity groups, accumulate)
        assert fn() == 0 and fn(grp=1) == 0 and fn(grp=12) == 0 and fn(acc=1) == 0
    L.call("fcn_device_sync")
