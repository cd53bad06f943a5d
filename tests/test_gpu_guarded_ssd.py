"""Guard-banded, poisoned-buffer tests of the SSD head's kernels (csrc/ssd.hip) against tests/ref_ssd64.py, -m gpu.

The gather is a copy and is held to exact equality; Normalize to the allowance of a C-term float32 sum; the row softmax to the bound
tests/test_gpu_guarded.py uses for the channel softmax; DetectionOutput to the same rows as the float64 reference - the same count, the
same (image, label) in the same order, score and corners within 1e-5 (the score, a copy of the bottom's, also bit for bit) - on inputs
whose decision margin tests/test_ssd_ref.py asserts, with what each case reaches: negative scores, no threshold, no background label,
300 classes.  Two cases run again with `capacity` exactly what the images can yield and the rows against the red zone."""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref_ssd64 as R
import ssd_cases
from fcn_object_detector_amd import lib as L
from gpu_util import POISON_WORD, g, launched_twice, poison_free, poisoned  # noqa: F401  (g is a fixture)

pytestmark = pytest.mark.gpu

HEADS = {   # (C, cstride, coffset, H, W)
    1: [(63, 64, 0, 19, 19)],
    2: [(12, 12, 0, 3, 5), (12, 12, 0, 19, 19)],
    3: [(6, 8, 2, 1, 1), (12, 12, 0, 3, 5), (63, 64, 0, 19, 19)],
    6: [(12, 12, 0, 3, 5), (63, 64, 0, 19, 19), (6, 8, 2, 1, 1), (12, 12, 0, 19, 19), (63, 64, 0, 3, 5), (6, 8, 0, 3, 5)],
}


def within(y, y64, allow, what=""):
    ratio, at = ref64.worst(y, y64, allow)
    print("BOUND %s %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (what, at, ratio)


def is_poison(a):
    return np.ascontiguousarray(a).view(np.uint32) == POISON_WORD


@pytest.mark.parametrize("nheads,start,gap,pad", [(1, 3, 0, 5), (3, 3, 7, 1), (6, 3, 0, 0), (6, 4, 4, 4), (2, 4, 8, 0)])
def test_gather(g, nheads, start, gap, pad):
    """Heads of C = 6, 12 and 63 over 1x1, 3x5 and 19x19 maps into rows that start at an odd (3) or an aligned (4) column, with `gap`
    untouched columns between heads and `pad` behind the row: (2, 4, 8, 0) moves 16 bytes per lane, the odd starts single floats."""
    rng = np.random.default_rng(100 + nheads)
    n = 2
    arr = (L.SsdHead * nheads)()
    xs, col, keep = [], start, []
    for h, (c, cs, co, hh, ww) in zip(arr, HEADS[nheads]):
        x = rng.standard_normal((n, c, hh, ww)).astype(np.float32)
        wide = poisoned((n, hh, ww, cs))
        wide[..., co:co + c] = x.transpose(0, 2, 3, 1)
        xd = g.put(wide, at_end=True, name="head")
        h.src, h.pixels, h.C, h.cstride, h.coffset, h.dst_col = xd.ptr, hh * ww, c, cs, co, col
        xs.append(x)
        keep.append((col, hh * ww * c, xd))
        col += hh * ww * c + gap
    cols = col - gap
    rstride = cols + pad
    yd = g.put(poisoned((n, rstride)), name="dst")
    out = launched_twice(lambda: L.call("fcn_ssd_gather_f32", arr, nheads, n, yd.ptr, rstride, cols, None), lambda: yd.read((n, rstride)))
    written = np.zeros(rstride, bool)
    for x, (c0, width, xd) in zip(xs, keep):
        assert np.array_equal(out[:, c0:c0 + width], R.gather([x]).astype(np.float32)), "head at column %d" % c0
        written[c0:c0 + width] = True
        assert xd.unchanged()
    assert poison_free(out[:, written]) and np.all(is_poison(out[:, ~written])), "columns outside the heads were written"


@pytest.mark.parametrize("shared", [0, 1])
@pytest.mark.parametrize("pixels", [1, 33])
@pytest.mark.parametrize("c", [5, 8, 70, 512])
def test_normalize(g, c, pixels, shared):
    rng = np.random.default_rng(200 + c)
    c4 = (c + 3) // 4 * 4
    xcs, xo, ycs, yo = c4 + 4, 1, c4 + 8, 4
    x = rng.standard_normal((pixels, c)).astype(np.float32) * 3
    scale = (rng.random(1 if shared else c) * 20 + 1).astype(np.float32)
    wide = poisoned((pixels, xcs))
    wide[:, xo:xo + c] = x
    xd, sd = g.put(wide, at_end=True, name="x"), g.put(scale, at_end=True, name="scale")
    yd = g.put(poisoned((pixels, ycs)), name="y")
    out = launched_twice(lambda: L.call("fcn_normalize_fwd_f32", xd.ptr, yd.ptr, sd.ptr, pixels, c, xcs, xo, ycs, yo, shared, 1e-10, None),
                         lambda: yd.read((pixels, ycs)))
    want = R.normalize(x.T[None, :, :, None], scale)[0, :, :, 0].T
    y = out[:, yo:yo + c]
    assert poison_free(y) and np.all(out[:, yo + c:yo + c4] == 0), "pad channels of the top are zeros"
    assert np.all(is_poison(out[:, :yo])) and np.all(is_poison(out[:, yo + c4:]))
    # the sum of C squares carries the sqrt(C) allowance of a float32 sum (halved by the root), then a root, a division and a product
    within(y, want, np.abs(want) * (0.5 * ref64.dot_bound_rms(c, 1.0) + 4 * ref64.U32) + 1e-37, "normalize C=%d" % c)
    assert xd.unchanged() and sd.unchanged()


@pytest.mark.parametrize("c", [3, 21])
def test_row_softmax(g, c):
    """fcn_softmax_fwd_f32 as the engine launches it for Softmax(axis 2) of an (N, P, C) blob: P rows of C dense floats, both strides C
    (no 16-byte alignment at C = 21 or 3), rows ending on the last byte in front of the red zone."""
    rng = np.random.default_rng(300 + c)
    rows = 33
    x = (rng.random((rows, c)) * 180 - 90).astype(np.float32)
    x[0] = 37.5
    xd, yd = g.put(x, at_end=True, name="x"), g.put(poisoned((rows, c)), at_end=True, name="y")
    L.call("fcn_softmax_fwd_f32", xd.ptr, yd.ptr, rows, c, c, c, None)
    y = yd.read((rows, c))
    want = R.row_softmax(x)
    assert poison_free(y) and xd.unchanged()
    within(y, want, (200 + c) * ref64.U32 * want + 1e-44, "row softmax C=%d" % c)


def det_params(c, n, loc_rs, conf_rs, cap):
    par = L.DetOutParams()
    par.N, par.P, par.num_classes, par.background = n, c["P"], c["classes"], c["bg"]
    par.code_type, par.variance_encoded, par.top_k, par.keep_top_k = c["code"], int(c["var_enc"]), c["top_k"], c["keep_top_k"]
    par.conf_threshold, par.nms_threshold, par.loc_rstride, par.conf_rstride, par.capacity = c["thr"], c["nms"], loc_rs, conf_rs, cap
    return par


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_detection_output(g, name, exact=False):
    """exact: `capacity` is what the images can yield and not a row more, and the rows end on the last byte in front of the red zone."""
    lib = L.load()
    c, loc, conf, priors, want, margin, count = ssd_cases.reference(name)
    assert margin >= ssd_cases.MARGIN      # (tests/test_ssd_ref.py asserts the same without a GPU)
    n, p, nc = c["N"], c["P"], c["classes"]
    loc_rs, conf_rs = p * 4 + 4, (p * nc + 3) // 4 * 4 + 4
    wl, wc = poisoned((n, loc_rs)), poisoned((n, conf_rs))
    wl[:, :p * 4], wc[:, :p * nc] = loc, conf
    per_class = min(c["top_k"], p) if c["top_k"] > -1 else p
    keep = c["keep_top_k"] if c["keep_top_k"] > -1 else (nc - (1 if c["bg"] >= 0 else 0)) * per_class
    cap = n * keep + (0 if exact else 3)
    par = det_params(c, n, loc_rs, conf_rs, cap)
    nbytes = int(lib.fcn_detection_output_workspace_bytes(C.byref(par)))
    assert nbytes > 0
    if exact:      # one row less is refused, so `cap` is the bound itself
        par.capacity = cap - 1
        assert int(lib.fcn_detection_output_workspace_bytes(C.byref(par))) == 0
        par.capacity = cap
    ld, cd, pd = g.put(wl, name="loc"), g.put(wc, name="conf"), g.put(priors, at_end=True, name="priors")
    od, nd, ws = g.put(poisoned((cap, 7)), at_end=exact, name="rows"), g.put(poisoned(1), at_end=True, name="count"), g.put(nbytes, name="workspace")
    rows, cnt = launched_twice(lambda: L.call("fcn_detection_output_f32", ld.ptr, cd.ptr, pd.ptr, C.byref(par), od.ptr, nd.ptr, ws.ptr, nbytes, None),
                               lambda: (od.read((cap, 7)), nd.read((1,), np.int32)))
    k = int(cnt[0])
    print("DETOUT %s count %d (reference %d) margin %.3g" % (name, k, count, margin))
    assert k == count
    assert np.all(is_poison(rows[k:])), "rows at and past the count were written"
    assert ld.unchanged() and cd.unchanged() and pd.unchanged()
    if count:
        got = rows[:k]
        assert poison_free(got)
        assert np.array_equal(got[:, :2], want[:, :2]), "image / label of the rows, in order"
        err = float(np.max(np.abs(got[:, 2:].astype(np.float64) - want[:, 2:])))
        print("DETOUT %s worst |error| %.3g" % (name, err))
        assert err <= 1e-5
        # a score is copied, not computed: the sign of a zero is the bottom's
        assert np.array_equal(bits(got[:, 2]), bits(want[:, 2])), "the rows' scores, bit for bit"


@pytest.mark.parametrize("name", list(ssd_cases.CASES))
def test_detection_output(g, name):
    run_detection_output(g, name)


@pytest.mark.parametrize("name", ssd_cases.EXACT_CAPACITY)
def test_detection_output_at_exact_capacity(g, name):
    run_detection_output(g, name, exact=True)
