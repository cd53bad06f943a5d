"""Guard-banded, poisoned-buffer parity of the Crop kernels against the float64 reference (tests/ref_crop64.py), -m gpu.

Both views are channel slices of wider pixels whose other channels hold NaN poison, with 256 KiB red zones around each payload
(tests/gpu_util.py); x ends on the last byte in front of its back red zone.  A copy has no rounding: results are compared for
exact equality, every case is launched twice and must give identical bits, and the poison shows a read outside the window (it
would arrive in y) as well as a write outside the slice."""
import numpy as np
import pytest

import ref_crop64 as R
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu
E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


# n, c, h, w, off_y, off_x, oh, ow, x_cstride, x_coffset, y_cstride, y_coffset   (float32 strides; the half cases double them)
CASES = [
    (2, 5, 7, 9, 0, 0, 7, 9, 8, 0, 8, 0),           # the whole blob
    (2, 5, 7, 9, 2, 0, 4, 9, 8, 0, 8, 0),           # offset in y only
    (2, 5, 7, 9, 0, 3, 7, 5, 8, 0, 8, 0),           # offset in x only
    (2, 5, 7, 9, 3, 4, 4, 5, 8, 0, 8, 0),           # window touching the far edges of both axes
    (1, 1, 6, 5, 1, 2, 3, 2, 4, 0, 4, 0),           # C = 1 in a pixel of 4
    (3, 3, 5, 6, 1, 1, 3, 4, 4, 0, 8, 4),           # C = 3, y at an aligned channel offset
    (1, 21, 12, 13, 5, 5, 6, 7, 24, 0, 24, 0),      # the published nets' 21 classes in pixels of 24: five whole groups and one channel
    (2, 64, 4, 5, 1, 2, 2, 3, 64, 0, 64, 0),        # whole groups only, dense pixels
    (1, 64, 4, 5, 1, 2, 2, 3, 136, 64, 72, 8),      # channel slices on both sides, aligned: the vector path
    (2, 6, 5, 4, 1, 1, 4, 3, 12, 3, 8, 1),          # a crop along the channel axis (x_coffset 3) into an unaligned slice: one lane per element
    (1, 8, 3, 3, 0, 1, 3, 2, 16, 8, 12, 2),         # aligned source, unaligned destination
    (1, 4, 40, 70, 9, 9, 22, 50, 4, 0, 4, 0),       # more lanes than one workgroup, rows that start at every 16-byte phase of a cache line
]


def run_twice(call, read):
    call()
    a = read()
    call()
    b = read()
    assert a.tobytes() == b.tobytes(), "two launches differ"
    return a


@pytest.mark.parametrize("dt", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", CASES)
def test_crop_forward(g, case, dt):
    n, c, h, w, oy, ox, oh, ow, xcs, xco, ycs, yco = case
    if dt is np.float16:
        xcs, xco, ycs, yco = 2 * xcs, 2 * xco, 2 * ycs, 2 * yco      # the same byte geometry: groups of 8 halves
        if case[9] % 4 or case[11] % 4:
            xco, yco = case[9], case[11]                              # keep the unaligned cases unaligned
    x = np.random.default_rng(CASES.index(case)).standard_normal((n, c, h, w)).astype(dt)
    xd = g.put(poisoned_nhwc(x, xcs, xco, dtype=dt), at_end=True, name="x")
    yd = g.put(poisoned((n, oh, ow, ycs), dtype=dt), name="y")
    name = "fcn_crop_fwd_f16" if dt is np.float16 else "fcn_crop_fwd_f32"
    full = run_twice(lambda: L.call(name, xd.ptr, yd.ptr, n, h, w, c, xcs, xco, oy, ox, oh, ow, ycs, yco, None), lambda: yd.read((n, oh, ow, ycs), dt))
    y = nchw(full, c, yco)
    assert poison_free(y), "poison from outside the window / the slice of x reached y"
    assert np.array_equal(y.astype(np.float64), R.crop(x, (0, 0, oy, ox), (n, c, oh, ow)))
    assert slice_untouched(full, yco, c), "channels of y outside the slice were written"


@pytest.mark.parametrize("case", CASES)
def test_crop_backward_plain_and_accumulating(g, case):
    n, c, h, w, oy, ox, oh, ow, xcs, xco, ycs, yco = case
    rng = np.random.default_rng(50 + CASES.index(case))
    dy = rng.standard_normal((n, c, oh, ow)).astype(np.float32)
    base = rng.standard_normal((n, c, h, w)).astype(np.float32)
    dyd = g.put(poisoned_nhwc(dy, ycs, yco), at_end=True, name="dy")
    args = (n, h, w, c, xcs, xco, oy, ox, oh, ow, ycs, yco)
    # plain: ONE launch over a poison-filled dX leaves dY inside the window and exact zeros outside it
    dxd = g.put(poisoned((n, h, w, xcs)), at_end=True, name="dx")
    full = run_twice(lambda: L.call("fcn_crop_bwd_f32", dyd.ptr, dxd.ptr, *args, 0, None), lambda: dxd.read((n, h, w, xcs)))
    got = nchw(full, c, xco)
    assert poison_free(got) and slice_untouched(full, xco, c)
    assert np.array_equal(got.astype(np.float64), R.crop_bwd(dy, (0, 0, oy, ox), (n, c, h, w)))
    # accumulating: += dY inside; outside the window dX keeps its bits - shown by poison there, which any read-modify-write
    # or store would have replaced or which would fail the bit comparison
    inside = np.zeros((n, c, h, w), bool)
    inside[:, :, oy:oy + oh, ox:ox + ow] = True
    start = np.where(inside, base, np.float32(np.nan))
    image = poisoned_nhwc(start, xcs, xco)
    dxa = g.put(image, at_end=True, name="dx (accumulate)")
    L.call("fcn_crop_bwd_f32", dyd.ptr, dxa.ptr, *args, 1, None)
    full = dxa.read((n, h, w, xcs))
    got = nchw(full, c, xco)
    want = R.crop_bwd(dy, (0, 0, oy, ox), (n, c, h, w), dx=np.where(inside, base, 0.0)).astype(np.float32)      # one correctly rounded add
    assert np.array_equal(got[inside], want[inside])
    keep = np.ones(full.shape, bool)
    keep[..., xco:xco + c] &= ~inside.transpose(0, 2, 3, 1)
    assert np.array_equal(full.view(np.uint32)[keep], image.view(np.uint32)[keep]), "accumulate touched dX outside the window"
    L.call("fcn_crop_bwd_f32", dyd.ptr, dxa.ptr, *args, 1, None)      # a second fan-in: dX + 2 dY in the order (dX + dY) + dY
    twice = nchw(dxa.read((n, h, w, xcs)), c, xco)
    assert np.array_equal(twice[inside], R.crop_bwd(dy, (0, 0, oy, ox), (n, c, h, w), dx=want).astype(np.float32)[inside])


def test_refusals_leave_the_buffers_alone(g):
    x = np.zeros((1, 4, 5, 6), np.float32)
    xd, yd = g.put(poisoned_nhwc(x, 8, 0), name="x"), g.put(poisoned((1, 3, 4, 8)), name="y")
    lib = L.load()
    ok = (1, 5, 6, 4, 8, 0, 1, 1, 3, 4, 8, 0)

    def variants(**kw):
        names = ("N", "H", "W", "C", "xcs", "xco", "oy", "ox", "OH", "OW", "ycs", "yco")
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    for fn in (lib.fcn_crop_fwd_f32, lib.fcn_crop_fwd_f16):
        assert fn(None, yd.ptr, *ok, None) == E_ARG and fn(xd.ptr, None, *ok, None) == E_ARG
        for bad in (dict(N=0), dict(C=0), dict(OH=0), dict(oy=3), dict(ox=3), dict(OW=6), dict(oy=-1), dict(xco=5), dict(yco=8)):
            assert fn(xd.ptr, yd.ptr, *variants(**bad), None) == E_ARG, bad
        assert fn(xd.ptr + 4, yd.ptr, *ok, None) == E_ALIGN and fn(xd.ptr, yd.ptr + 8, *ok, None) == E_ALIGN
        assert fn(xd.ptr, yd.ptr, *variants(xcs=10, C=2), None) == E_ALIGN and fn(xd.ptr, yd.ptr, *variants(ycs=12 if fn is lib.fcn_crop_fwd_f16 else 10, C=2), None) == E_ALIGN
        assert fn(xd.ptr, yd.ptr, *variants(N=1 << 12, H=1 << 10, W=1 << 10), None) == E_UNSUPPORTED
    assert lib.fcn_crop_bwd_f32(None, xd.ptr, *ok, 0, None) == E_ARG and lib.fcn_crop_bwd_f32(yd.ptr, None, *ok, 0, None) == E_ARG
    assert lib.fcn_crop_bwd_f32(yd.ptr, xd.ptr, *ok, 2, None) == E_ARG
    assert lib.fcn_crop_bwd_f32(yd.ptr, xd.ptr, *variants(oy=3), 0, None) == E_ARG
    assert lib.fcn_crop_bwd_f32(yd.ptr + 4, xd.ptr, *ok, 1, None) == E_ALIGN
    assert lib.fcn_crop_bwd_f32(yd.ptr, xd.ptr, *variants(N=1 << 12, H=1 << 10, W=1 << 10), 0, None) == E_UNSUPPORTED
    L.call("fcn_device_sync")
    assert xd.unchanged() and yd.unchanged()
