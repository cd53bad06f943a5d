"""Guard-banded, poisoned-buffer parity of the Interp kernels against the float64 reference (tests/ref_interp64.py), -m gpu.

Both views are channel slices of wider pixels whose other channels hold NaN poison, with 256 KiB red zones around each payload
(tests/gpu_util.py); inputs end on the last byte in front of their back red zone and must be bit-identical after the launch; every
case is launched twice and must give identical bits.  The poison shows a read outside the channel window or outside the effective
input (the rim that pad_beg / pad_end crop holds NaN too) as well as a write outside the slice.

Bounds (tests/ref64.py): forward dot_bound(6, interpolation of |x|) - four products of three factors and the weights' own roundings;
half outputs dot_bound_f16 of the same; backward dot_bound(6 + F, adjoint of |dY|) with F the largest number of output pixels that
feed one input pixel, counted from the reference's weight matrices (225 for 5 x 7 -> 33 x 49).  Outputs that fall on an input pixel
(equal extents, 17 -> 3) are compared for exact equality."""
import numpy as np
import pytest

import ref64
import ref_interp64 as R
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd.engine import DeviceBuffer
from gpu_util import DeviceMemory, Guards, dev_from, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu
E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
N = 2

# h, w, oh, ow, pad_beg, pad_end
SHAPES = [(5, 7, 33, 49, 0, 0), (1, 1, 6, 6, 0, 0), (2, 3, 6, 6, 0, 0), (6, 6, 6, 6, 0, 0), (9, 11, 3, 4, 0, 0), (17, 17, 3, 3, 0, 0),
          (3, 1, 7, 5, 0, 0), (7, 9, 1, 1, 0, 0), (4, 5, 1, 6, 0, 0),
          (9, 9, 9, 9, -1, -2)]       # cropped: 6 x 6 effective, shrink 2 then zoom 4
# c, x_cstride, x_coffset, y_cstride, y_coffset
LAYOUTS = [(1, 4, 0, 4, 0), (3, 4, 0, 4, 0), (5, 8, 0, 8, 0), (21, 24, 0, 24, 0),      # the scalar tail behind whole segments; NaN pad channels
           (8, 16, 4, 16, 4),                                                           # whole segments inside a window
           (6, 12, 3, 10, 1)]                                                           # nothing aligned: one lane per element
EXACT = [(6, 6, 6, 6, 0, 0), (17, 17, 3, 3, 0, 0)]


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def ids(v):
    return "-".join(str(a) for a in v)


def run_twice(call, read):
    call()
    a = read()
    call()
    b = read()
    assert a.tobytes() == b.tobytes(), "two launches differ"
    return a


def rim_poisoned(x, pb, pe):
    """x with NaN in the rows and columns that the pads crop away."""
    out = np.full(x.shape, np.nan, x.dtype)
    h, w = x.shape[2:]
    out[:, :, -pb:h + pe, -pb:w + pe] = x[:, :, -pb:h + pe, -pb:w + pe]
    return out


def exact_want(x, shape):
    h, w, oh, ow, pb, pe = shape
    return x if oh == h else x[:, :, ::(h - 1) // (oh - 1), ::(w - 1) // (ow - 1)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=ids)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_interp_forward_f32(g, shape, layout):
    h, w, oh, ow, pb, pe = shape
    c, xcs, xco, ycs, yco = layout
    x = rim_poisoned(np.random.default_rng(SHAPES.index(shape) * 10 + c).standard_normal((N, c, h, w)).astype(np.float32), pb, pe)
    xd = g.put(poisoned_nhwc(x, xcs, xco), at_end=True, name="x")
    yd = g.put(poisoned((N, oh, ow, ycs)), name="y")
    full = run_twice(lambda: L.call("fcn_interp_fwd_f32", xd.ptr, yd.ptr, N, h, w, c, xcs, xco, pb, pe, oh, ow, ycs, yco, None),
                     lambda: yd.read((N, oh, ow, ycs)))
    y = nchw(full, c, yco)
    assert poison_free(y), "poison from outside the effective input / the slice of x reached y"
    assert slice_untouched(full, yco, c), "channels of y outside the slice were written"
    assert xd.unchanged()
    clean = np.nan_to_num(x.astype(np.float64))
    y64, mag = R.interp(clean, oh, ow, pb, pe), R.interp_mag(clean, oh, ow, pb, pe)
    r, at = ref64.worst(y, y64, ref64.dot_bound(6, mag))
    print("interp fwd %s %s: worst |err| / bound %.3g" % (ids(shape), ids(layout), r))
    assert r <= 1.0, (r, at)
    if shape in EXACT:
        assert y.tobytes() == np.ascontiguousarray(exact_want(x, shape)).tobytes(), "an output on an input pixel is that pixel, bit for bit"


# c, x_cstride, x_coffset, y_cstride, y_coffset, out_f32
HALF_LAYOUTS = [(8, 16, 8, 16, 0, 0), (24, 24, 0, 32, 8, 0), (5, 8, 0, 8, 0, 1), (21, 24, 0, 24, 0, 0), (8, 8, 0, 12, 4, 1)]


@pytest.mark.parametrize("layout", HALF_LAYOUTS, ids=ids)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_interp_forward_f16(g, shape, layout):
    h, w, oh, ow, pb, pe = shape
    c, xcs, xco, ycs, yco, out_f32 = layout
    odt = np.float32 if out_f32 else np.float16
    x = rim_poisoned(np.random.default_rng(SHAPES.index(shape) * 10 + c).standard_normal((N, c, h, w)).astype(np.float16), pb, pe)
    xd = g.put(poisoned_nhwc(x, xcs, xco, dtype=np.float16), at_end=True, name="x")
    yd = g.put(poisoned((N, oh, ow, ycs), dtype=odt), name="y")
    full = run_twice(lambda: L.call("fcn_interp_fwd_f16", xd.ptr, yd.ptr, N, h, w, c, xcs, xco, pb, pe, oh, ow, ycs, yco, out_f32, None),
                     lambda: yd.read((N, oh, ow, ycs), odt))
    y = nchw(full, c, yco)
    assert poison_free(y) and slice_untouched(full, yco, c) and xd.unchanged()
    clean = np.nan_to_num(x.astype(np.float64))
    y64, mag = R.interp(clean, oh, ow, pb, pe), R.interp_mag(clean, oh, ow, pb, pe)
    allow = ref64.dot_bound(6, mag) if out_f32 else ref64.dot_bound_f16(6, mag, y64)
    r, at = ref64.worst(y, y64, allow)
    print("interp fwd f16 %s %s: worst |err| / bound %.3g" % (ids(shape), ids(layout), r))
    assert r <= 1.0, (r, at)
    if shape in EXACT:
        assert np.array_equal(y.astype(np.float64), exact_want(x, shape).astype(np.float64))


@pytest.mark.parametrize("layout", LAYOUTS, ids=ids)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_interp_backward_plain_and_accumulating(g, shape, layout):
    h, w, oh, ow, pb, pe = shape
    c, xcs, xco, ycs, yco = layout
    rng = np.random.default_rng(500 + SHAPES.index(shape) * 10 + c)
    dy = rng.standard_normal((N, c, oh, ow)).astype(np.float32)
    base = rng.standard_normal((N, c, h, w)).astype(np.float32)
    dyd = g.put(poisoned_nhwc(dy, ycs, yco), at_end=True, name="dy")
    args = (N, h, w, c, xcs, xco, pb, pe, oh, ow, ycs, yco)
    K = 6 + R.max_feeders(h, w, oh, ow, pb, pe)
    fed = np.broadcast_to(R.fed(h, w, oh, ow, pb, pe), (N, c, h, w))
    want, mag = R.interp_bwd(dy, h, w, pb, pe), R.interp_bwd_mag(dy, h, w, pb, pe)
    # plain: ONE launch over a poison-filled dX leaves the sums where something feeds a pixel and exact zeros elsewhere
    dxd = g.put(poisoned((N, h, w, xcs)), at_end=True, name="dx")
    full = run_twice(lambda: L.call("fcn_interp_bwd_f32", dyd.ptr, dxd.ptr, *args, 0, None), lambda: dxd.read((N, h, w, xcs)))
    got = nchw(full, c, xco)
    assert poison_free(got) and slice_untouched(full, xco, c) and dyd.unchanged()
    r, at = ref64.worst(got, want, ref64.dot_bound(K, mag))
    print("interp bwd %s %s: K %d, worst |err| / bound %.3g" % (ids(shape), ids(layout), K, r))
    assert r <= 1.0, (r, at)
    assert not got[~fed].view(np.uint32).any(), "a pixel that nothing feeds is +0.0"
    # accumulating: += the sums where something feeds a pixel; everything else keeps its bits - shown by poison there
    start = np.where(fed, base, np.float32(np.nan))
    image = poisoned_nhwc(start, xcs, xco)
    dxa = g.put(image, at_end=True, name="dx (accumulate)")
    L.call("fcn_interp_bwd_f32", dyd.ptr, dxa.ptr, *args, 1, None)
    full = dxa.read((N, h, w, xcs))
    got = nchw(full, c, xco)
    want_acc = R.interp_bwd(dy, h, w, pb, pe, dx=np.where(fed, base, 0.0))
    r, at = ref64.worst(got[fed], want_acc[fed], ref64.dot_bound(K, mag + np.abs(base))[fed])
    assert r <= 1.0, (r, at)
    keep = np.ones(full.shape, bool)
    keep[..., xco:xco + c] &= ~fed.transpose(0, 2, 3, 1)
    assert np.array_equal(full.view(np.uint32)[keep], image.view(np.uint32)[keep]), "accumulate touched dX where nothing feeds it"
    assert dyd.unchanged()


def test_an_output_past_two_to_the_31_bytes(gpu):
    """33 -> 257 (zoom_factor 8) into pixels of 4096 floats: the last output pixel lies 2.16e9 bytes into y.  Only the first and the
    last output row are read back."""
    c, h, oh, ycs = 4, 33, 257, 4096
    yco = ycs - c
    x = np.random.default_rng(7).standard_normal((N, c, h, h)).astype(np.float32)
    xd = dev_from(poisoned_nhwc(x, 4, 0))
    row_bytes = oh * ycs * 4
    total = N * oh * row_bytes
    assert total > 1 << 31
    yd = DeviceBuffer(total, zero=True)
    try:
        mem = DeviceMemory()
        L.call("fcn_interp_fwd_f32", xd.ptr, yd.ptr, N, h, h, c, 4, 0, 0, 0, oh, oh, ycs, yco, None)
        L.call("fcn_device_sync")
        y64 = R.interp(x, oh, oh)
        allow = ref64.dot_bound(6, R.interp_mag(x, oh, oh))
        for n, oy, off in ((0, 0, 0), (N - 1, oh - 1, total - row_bytes)):
            row = mem.download(yd, off, row_bytes).view(np.float32).reshape(oh, ycs)
            got = row[:, yco:].T                                     # (c, ow)
            r, at = ref64.worst(got, y64[n, :, oy, :], allow[n, :, oy, :])
            assert r <= 1.0, (n, oy, r, at)
        assert not row[:, :yco].view(np.uint32).any(), "the last row's other channels keep their zeros"
    finally:
        yd.free()
        xd.free()


def test_refusals_leave_the_buffers_alone(g):
    x = np.zeros((1, 4, 5, 6), np.float32)
    xd, yd = g.put(poisoned_nhwc(x, 8, 0), name="x"), g.put(poisoned((1, 9, 11, 8)), name="y")
    lib = L.load()
    ok = (1, 5, 6, 4, 8, 0, 0, 0, 9, 11, 8, 0)

    def variants(**kw):
        names = ("N", "H", "W", "C", "xcs", "xco", "pb", "pe", "OH", "OW", "ycs", "yco")
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    calls = {"fcn_interp_fwd_f32": lambda a, b, v: lib.fcn_interp_fwd_f32(a, b, *v, None),
             "fcn_interp_fwd_f16": lambda a, b, v: lib.fcn_interp_fwd_f16(a, b, *v, 0, None),
             "fcn_interp_bwd_f32": lambda a, b, v: lib.fcn_interp_bwd_f32(b, a, *v, 0, None)}
    for name, fn in calls.items():
        assert fn(None, yd.ptr, ok) == E_ARG and fn(xd.ptr, None, ok) == E_ARG, name
        for bad in (dict(N=0), dict(C=0), dict(OH=0), dict(W=0), dict(pb=1), dict(pe=2), dict(pb=-2, pe=-3), dict(xco=5), dict(yco=8)):
            assert fn(xd.ptr, yd.ptr, variants(**bad)) == E_ARG, (name, bad)
        assert fn(xd.ptr, yd.ptr, variants(OW=(1 << 24) + 1)) == E_UNSUPPORTED, name
    assert lib.fcn_interp_fwd_f16(xd.ptr, yd.ptr, *variants(xcs=12), 0, None) == E_ALIGN
    assert lib.fcn_interp_fwd_f16(xd.ptr, yd.ptr, *variants(yco=2, C=2), 1, None) == E_ALIGN
    assert lib.fcn_interp_fwd_f16(xd.ptr + 8, yd.ptr, *ok, 0, None) == E_ALIGN
    assert lib.fcn_interp_fwd_f16(xd.ptr, yd.ptr, *ok, 3, None) == E_ARG
    assert lib.fcn_interp_bwd_f32(yd.ptr, xd.ptr, *ok, 2, None) == E_ARG
    L.call("fcn_device_sync")
    assert xd.unchanged() and yd.unchanged()
