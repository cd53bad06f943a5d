"""Guard-banded, poisoned-buffer parity of the Upsample kernels, the half MAX pooling with argmax and the mask read-back against
tests/ref_unpool64.py, -m gpu.

Every view is a channel slice of wider pixels whose other channels hold NaN poison, with 256 KiB red zones around each payload
(tests/gpu_util.py); inputs end on the last byte in front of their back red zone and must be bit-identical after the launch; every
forward case is launched twice and must give identical bits.  The kernels move values and do no arithmetic, so every comparison is
for EXACT equality, zeros included (+0.0); the one float32 add of an accumulating backward is performed in float32 by the reference.

Shapes are the smallest that still reach every path: 7 x 9 under 2 x 2 / 2 pools to 4 x 5 in ceil mode with clipped edge windows;
3 x 3 / 2 (pad 0 and 1) over small integers makes neighbouring windows share an argmax (asserted on the CPU), which pins the
last-writer rule and the zero fill; C = 6 is a partial 16-byte group of floats and a partial 8-half segment; C = 20 sits at offset 8 of
40-channel pixels; N = 2 on 6 x 8 with C = 40 puts the end of one image and the start of the next into one block of lanes; a
y_coffset of 2 in pixels of an odd stride takes the element-wise stores."""
import numpy as np
import pytest

import ref_unpool64 as R
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu
E_ARG, E_ALIGN = 1, 2

# n, h, w, k, stride, pad
GEOMS = [(1, 7, 9, 2, 2, 0), (1, 7, 9, 3, 2, 0), (1, 7, 9, 3, 2, 1), (2, 6, 8, 2, 2, 0)]
# c, x_cstride, x_coffset, y_cstride, y_coffset
LAYOUTS = [(6, 8, 0, 8, 0), (20, 40, 8, 40, 8), (40, 40, 0, 40, 0), (5, 7, 1, 9, 2), (8, 8, 0, 11, 2)]
# c, x_cstride, x_coffset, y_cstride, y_coffset, out_f32
HALF_LAYOUTS = [(6, 8, 0, 8, 0, 0), (20, 40, 8, 40, 8, 0), (40, 40, 0, 40, 0, 0), (6, 8, 0, 9, 2, 1), (20, 40, 8, 40, 8, 1), (16, 16, 0, 9 + 16, 2, 1)]


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


def packed(idx):
    """(N, C, PH, PW) -> the kernels' [N * PH * PW][C] int32."""
    return np.ascontiguousarray(idx.transpose(0, 2, 3, 1)).astype(np.int32)


def mask_for(geom, c, seed, dtype=np.float32):
    """The argmax of a MAX pooling over small integers (3 x 3 windows: neighbours then share argmaxes - asserted) or over normal
    values (2 x 2 / 2: windows are disjoint)."""
    n, h, w, k, s, p = geom
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 3, (n, c, h, w)).astype(dtype) if k > s else rng.standard_normal((n, c, h, w)).astype(dtype)
    _, idx = R.max_pool_argmax(src, k, s, p)
    assert idx.min() >= 0 and idx.max() < h * w
    dup = sum(np.unique(idx[i, j]).size < idx[i, j].size for i in range(n) for j in range(c))
    assert (dup > 0) == (k > s), "overlapping windows over a plateau must share argmaxes; disjoint windows cannot"
    return idx


@pytest.mark.parametrize("layout", LAYOUTS, ids=ids)
@pytest.mark.parametrize("geom", GEOMS, ids=ids)
def test_unpool_forward_f32(g, geom, layout):
    n, h, w, k, s, p = geom
    c, xcs, xco, ycs, yco = layout
    idx = mask_for(geom, c, GEOMS.index(geom) * 10 + c)
    ph, pw = idx.shape[2:]
    x = np.random.default_rng(c).standard_normal((n, c, ph, pw)).astype(np.float32)
    xd = g.put(poisoned_nhwc(x, xcs, xco), at_end=True, name="x")
    idd = g.put(packed(idx), at_end=True, name="idx")
    yd = g.put(poisoned((n, h, w, ycs)), name="y")
    full = run_twice(lambda: L.call("fcn_unpool_fwd_f32", xd.ptr, idd.ptr, yd.ptr, n, ph, pw, c, xcs, xco, k, s, p, h, w, ycs, yco, None),
                     lambda: yd.read((n, h, w, ycs)))
    y = nchw(full, c, yco)
    assert poison_free(y), "poison from the pad channels of x reached y, or an element of the slice was not written"
    assert slice_untouched(full, yco, c), "channels of y outside the slice were written"
    assert xd.unchanged() and idd.unchanged()
    want = R.unpool(x, idx, h, w)
    assert y.tobytes() == want.tobytes(), "unpool fwd %s %s: %d elements differ" % (ids(geom), ids(layout), int((y != want).sum()))


@pytest.mark.parametrize("layout", HALF_LAYOUTS, ids=ids)
@pytest.mark.parametrize("geom", GEOMS, ids=ids)
def test_unpool_forward_f16(g, geom, layout):
    n, h, w, k, s, p = geom
    c, xcs, xco, ycs, yco, out_f32 = layout
    odt = np.float32 if out_f32 else np.float16
    idx = mask_for(geom, c, 100 + GEOMS.index(geom) * 10 + c)
    ph, pw = idx.shape[2:]
    x = np.random.default_rng(c).standard_normal((n, c, ph, pw)).astype(np.float16)
    xd = g.put(poisoned_nhwc(x, xcs, xco, dtype=np.float16), at_end=True, name="x")
    idd = g.put(packed(idx), at_end=True, name="idx")
    yd = g.put(poisoned((n, h, w, ycs), dtype=odt), name="y")
    full = run_twice(lambda: L.call("fcn_unpool_fwd_f16", xd.ptr, idd.ptr, yd.ptr, n, ph, pw, c, xcs, xco, k, s, p, h, w, ycs, yco, out_f32, None),
                     lambda: yd.read((n, h, w, ycs), odt))
    y = nchw(full, c, yco)
    assert poison_free(y) and slice_untouched(full, yco, c) and xd.unchanged() and idd.unchanged()
    want = R.unpool(x, idx, h, w).astype(odt)                       # (half -> float32 is exact)
    assert y.tobytes() == want.tobytes(), "unpool fwd f16 %s %s: %d elements differ" % (ids(geom), ids(layout), int((y != want).sum()))


@pytest.mark.parametrize("layout", [(6, 8, 0, 8, 0), (20, 40, 8, 40, 8), (5, 7, 1, 9, 2)], ids=ids)
@pytest.mark.parametrize("geom", GEOMS, ids=ids)
def test_unpool_backward_plain_and_accumulating(g, geom, layout):
    n, h, w, k, s, p = geom
    c, xcs, xco, ycs, yco = layout
    idx = mask_for(geom, c, 200 + GEOMS.index(geom) * 10 + c)
    ph, pw = idx.shape[2:]
    rng = np.random.default_rng(300 + c)
    dy = rng.standard_normal((n, c, h, w)).astype(np.float32)
    base = rng.standard_normal((n, c, ph, pw)).astype(np.float32)
    dyd = g.put(poisoned_nhwc(dy, ycs, yco), at_end=True, name="dy")
    idd = g.put(packed(idx), at_end=True, name="idx")
    args = (n, ph, pw, c, xcs, xco, k, s, p, h, w, ycs, yco)
    dxd = g.put(poisoned((n, ph, pw, xcs)), at_end=True, name="dx")
    full = run_twice(lambda: L.call("fcn_unpool_bwd_f32", dyd.ptr, idd.ptr, dxd.ptr, *args, 0, None), lambda: dxd.read((n, ph, pw, xcs)))
    got = nchw(full, c, xco)
    assert poison_free(got) and slice_untouched(full, xco, c) and dyd.unchanged() and idd.unchanged()
    assert got.tobytes() == R.unpool_bwd(dy, idx).tobytes()
    dxa = g.put(poisoned_nhwc(base, xcs, xco), at_end=True, name="dx (accumulate)")
    L.call("fcn_unpool_bwd_f32", dyd.ptr, idd.ptr, dxa.ptr, *args, 1, None)
    full = dxa.read((n, ph, pw, xcs))
    got = nchw(full, c, xco)
    assert poison_free(got) and slice_untouched(full, xco, c) and dyd.unchanged()
    assert got.tobytes() == R.unpool_bwd(dy, idx, dx=base).tobytes()


def test_an_index_outside_the_plane_moves_nothing(g):
    """-1 is what a window without a maximum holds: forward never matches it, backward gathers 0 for it (and reads nothing)."""
    n, h, w, c = 1, 4, 6, 4
    idx = np.full((n, c, 2, 3), -1, np.int32)
    idx[0, 1] = [[0, 2, 4], [12, 14, 16]]
    x = np.arange(1, 1 + idx.size, dtype=np.float32).reshape(idx.shape)
    xd, idd, yd = g.put(poisoned_nhwc(x, 4, 0), at_end=True), g.put(packed(idx), at_end=True), g.put(poisoned((n, h, w, 4)))
    L.call("fcn_unpool_fwd_f32", xd.ptr, idd.ptr, yd.ptr, n, 2, 3, c, 4, 0, 2, 2, 0, h, w, 4, 0, None)
    assert nchw(yd.read((n, h, w, 4)), c).tobytes() == R.unpool(x, idx, h, w).tobytes()
    dy = np.random.default_rng(1).standard_normal((n, c, h, w)).astype(np.float32)
    dyd, dxd = g.put(poisoned_nhwc(dy, 4, 0), at_end=True), g.put(poisoned((n, 2, 3, 4)))
    L.call("fcn_unpool_bwd_f32", dyd.ptr, idd.ptr, dxd.ptr, n, 2, 3, c, 4, 0, 2, 2, 0, h, w, 4, 0, 0, None)
    assert nchw(dxd.read((n, 2, 3, 4)), c).tobytes() == R.unpool_bwd(dy, idx).tobytes()


# c, x_cstride, y_cstride, y_coffset
@pytest.mark.parametrize("layout", [(8, 8, 8, 0), (24, 32, 40, 8)], ids=ids)
@pytest.mark.parametrize("plateau", [False, True], ids=["normal", "plateau"])
@pytest.mark.parametrize("geom", GEOMS, ids=ids)
def test_maxpool_idx_f16(g, geom, plateau, layout):
    """y bit for bit what fcn_maxpool_fwd_f16 gives on the same input; idx the reference's argmax of the half input (first maximum in
    raster order, clipped windows).  Pad channels and red zones of x hold +65504: a window that leaves its image or its channels wins."""
    n, h, w, k, s, p = geom
    c, xcs, ycs, yco = layout
    rng = np.random.default_rng(400 + GEOMS.index(geom) * 10 + c)
    x = (rng.integers(-2, 3, (n, c, h, w)) if plateau else rng.standard_normal((n, c, h, w))).astype(np.float16)
    want_y, want_idx = R.max_pool_argmax(x, k, s, p)
    oh, ow = want_y.shape[2:]
    xd = g.put(poisoned_nhwc(x, xcs, 0, poison="huge", dtype=np.float16), at_end=True, poison="huge", name="x")
    yd = g.put(poisoned((n, oh, ow, ycs), dtype=np.float16), name="y")
    y2 = g.put(poisoned((n, oh, ow, ycs), dtype=np.float16), name="y of fcn_maxpool_fwd_f16")
    idd = g.put(n * oh * ow * c * 4, name="idx")
    full = run_twice(lambda: L.call("fcn_maxpool_idx_fwd_f16", xd.ptr, yd.ptr, idd.ptr, n, h, w, c, xcs, k, s, p, oh, ow, ycs, yco, None),
                     lambda: yd.read((n, oh, ow, ycs), np.float16))
    L.call("fcn_maxpool_fwd_f16", xd.ptr, y2.ptr, n, h, w, c, xcs, k, s, p, oh, ow, ycs, yco, None)
    plain = y2.read((n, oh, ow, ycs), np.float16)
    assert full.tobytes() == plain.tobytes(), "y differs from fcn_maxpool_fwd_f16"
    y = nchw(full, c, yco)
    assert poison_free(y, "huge") and slice_untouched(full, yco, c) and xd.unchanged()
    assert y.tobytes() == want_y.tobytes()
    got_idx = idd.read((n, oh, ow, c), np.int32).transpose(0, 3, 1, 2)
    assert np.array_equal(got_idx, want_idx), "%d argmaxes differ" % int((got_idx != want_idx).sum())


@pytest.mark.parametrize("shape", [(1, 6, 4, 5), (2, 40, 3, 4), (3, 1, 1, 1)], ids=ids)
def test_pool_mask_to_nchw(g, shape):
    n, c, ph, pw = shape
    idx = np.random.default_rng(sum(shape)).integers(-1, 1 << 20, shape).astype(np.int32)
    idd = g.put(packed(idx), at_end=True, name="idx")
    dd = g.put(poisoned(shape), at_end=True, name="dst")
    got = run_twice(lambda: L.call("fcn_pool_mask_to_nchw_f32", idd.ptr, dd.ptr, n, ph, pw, c, None), lambda: dd.read(shape))
    assert got.tobytes() == R.mask_nchw(idx).tobytes() and idd.unchanged()


def test_refusals_leave_the_buffers_alone(g):
    x = np.zeros((1, 8, 4, 5), np.float32)
    xd, yd = g.put(poisoned_nhwc(x, 8, 0), name="x"), g.put(poisoned((1, 7, 9, 8)), name="y")
    idd = g.put(np.zeros((20, 8), np.int32), name="idx")
    lib = L.load()
    ok = (1, 4, 5, 8, 8, 0, 2, 2, 0, 7, 9, 8, 0)
    assert lib.fcn_unpool_fwd_f32(xd.ptr, idd.ptr, yd.ptr, *ok[:1], 3, *ok[2:], None) == E_ARG
    assert lib.fcn_unpool_fwd_f32(xd.ptr, None, yd.ptr, *ok, None) == E_ARG
    assert lib.fcn_unpool_fwd_f16(xd.ptr + 8, idd.ptr, yd.ptr, *ok, 0, None) == E_ALIGN
    assert lib.fcn_unpool_bwd_f32(yd.ptr, idd.ptr, xd.ptr, *ok, 2, None) == E_ARG
    assert lib.fcn_maxpool_idx_fwd_f16(yd.ptr, xd.ptr, idd.ptr, 1, 7, 9, 8, 8, 2, 2, 0, 4, 6, 8, 0, None) == E_ARG
    assert lib.fcn_pool_mask_to_nchw_f32(idd.ptr, yd.ptr + 2, 1, 4, 5, 8, None) == E_ALIGN
    L.call("fcn_device_sync")
    assert xd.unchanged() and yd.unchanged() and idd.unchanged()
