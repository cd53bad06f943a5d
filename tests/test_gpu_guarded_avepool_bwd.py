"""fcn_avepool_bwd_f32 in guard-banded, poisoned buffers against the float64 backward of tests/ref_avepool64.py.

The allowance of an element is that of a float32 sum over the windows that cover it (ref64.dot_bound_rms over their number, on the
magnitude term sum |dY| / divisor), one rounding for each quotient and one for the accumulated value - as the forward's guarded case
(tests/test_gpu_guarded.py, test_avepool_divisor_counts_the_padding) does it.  Every call runs twice: the two results are bit-equal."""
import numpy as np
import pytest

import ref64
import ref_avepool64
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def within(y, y64, allow, what=""):
    ratio, at = ref64.worst(y, y64, allow)
    print("BOUND %s %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (what, at, ratio)


# c, dy_cstride, dy_coffset, dx_cstride, dx_coffset: a window with poisoned channels on both sides in both blobs; C no multiple of 4
# (the last 16-byte group is stored in part) with a window; whole buffers
SLICES = [(8, 16, 4, 20, 8), (6, 12, 4, 16, 4), (5, 8, 0, 8, 0), (3, 4, 0, 12, 8), (16, 16, 0, 16, 0)]


@pytest.mark.parametrize("c,cs_dy,co_dy,cs_dx,co_dx", SLICES)
@pytest.mark.parametrize("k,s,p,h,w", ref_avepool64.CASES)
def test_avepool_backward(g, k, s, p, h, w, c, cs_dy, co_dy, cs_dx, co_dx):
    rng = np.random.default_rng(12)
    n = 2
    oh, ow = ref64.pool_out(h, k, p, s), ref64.pool_out(w, k, p, s)
    dy = (rng.standard_normal((n, c, oh, ow)) + 1.5).astype(np.float32)      # a mean far from zero: a wrong divisor shows
    base = rng.standard_normal((n, c, h, w)).astype(np.float32)
    want = ref_avepool64.ave_pool_bwd(dy, k, s, p, h, w)
    mag = ref_avepool64.ave_pool_bwd(np.abs(dy), k, s, p, h, w)
    cnt = ref_avepool64.cover_count(k, s, p, h, w)
    dyd = g.put(poisoned_nhwc(dy, cs_dy, co_dy), at_end=True, name="dy")
    args = (n, h, w, c, cs_dx, co_dx, k, s, p, oh, ow, cs_dy, co_dy)
    for acc in (0, 1):
        runs = []
        for rep in range(2):
            dxd = g.put(poisoned_nhwc(base, cs_dx, co_dx) if acc else poisoned((n, h, w, cs_dx)), at_end=True, name="dx acc=%d run %d" % (acc, rep))
            L.call("fcn_avepool_bwd_f32", dyd.ptr, dxd.ptr, *args, acc, None)
            L.call("fcn_device_sync")
            runs.append(dxd.read((n, h, w, cs_dx)))
        full = runs[0]
        assert np.array_equal(full.view(np.uint32), runs[1].view(np.uint32)), "two identical calls gave different bits"
        got = nchw(full, c, co_dx)
        ref = want + base.astype(np.float64) * acc
        assert poison_free(got) and slice_untouched(full, co_dx, c)
        allow = ref64.dot_bound_rms(cnt, mag) + ref64.U32 * (mag + np.abs(ref))
        within(got, ref, allow, "avepool bwd k%d s%d p%d %dx%d c%d acc=%d" % (k, s, p, h, w, c, acc))
        if acc:
            assert np.array_equal(got[:, :, cnt == 0], base[:, :, cnt == 0])      # pixels under no window stay as they are
        else:
            assert np.all(got[:, :, cnt == 0] == 0)                               # ... or get exact zeros
