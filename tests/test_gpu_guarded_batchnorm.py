"""The BatchNorm / Scale entry points (csrc/batchnorm.hip) in guard-banded, poisoned buffers against tests/ref_batchnorm64.py.

Allowances are derived, not tuned (ref64.dot_bound_rms / ref64.U32, as in the other guarded files): a reduction over the m values of a
channel gets the allowance of a float32 sum of m terms on ITS magnitude term, every further operation one rounding on the magnitude
of its result.
  mean      sum of m terms on sum |x| / m, two roundings
  variance  sum of m terms on sum (x - mean)^2 / m = the variance itself, four roundings, and the SQUARE of the mean's allowance: the
            deviations from the true mean sum to zero, so an error of the centre enters only at second order.  A kernel that forms
            E[x^2] - E[x]^2 has E[x^2] as its magnitude term and misses this allowance by construction once |mean| >> std
            (test_variance_is_centred: |mean| = 100 std); the float32 two-pass computation on the CPU stays inside it.
  invstd    the variance's allowance through d/dv (v + eps)^-1/2, three roundings
  apply     operands as given (float32): subtraction, two products, one sum; with global statistics the prologue's 1 / factor, the
            two products, the sum with eps, the square root and the quotient are counted on the terms they touch
  backward  the two sums: m terms on sum |dy'| and sum |dy' xhat|; the apply: the roundings of its five operations
Every call runs twice into fresh poisoned buffers and the two results are bit-equal."""
import numpy as np
import pytest

import ref64
import ref_batchnorm64 as R
from fcn_object_detector_amd import lib as L
from gpu_util import Guards, nchw, poison_free, poisoned, poisoned_nhwc, slice_untouched

pytestmark = pytest.mark.gpu
U = ref64.U32
F32 = np.float32


@pytest.fixture
def g(gpu):
    with Guards() as guards:
        yield guards


def within(y, y64, allow, what=""):
    ratio, at = ref64.worst(y, y64, allow)
    print("BOUND %s %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (what, at, ratio)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def ch(v):
    return np.asarray(v, np.float64).reshape(1, -1, 1, 1)


# c, cstride / coffset of the first view, cstride / coffset of the second: poisoned channels on both sides of every window, C no
# multiple of 4 (the last 16-byte group is stored in part), and a whole buffer
SLICES = [(3, 12, 4, 8, 4), (5, 16, 4, 12, 4), (6, 12, 4, 16, 4), (8, 16, 4, 20, 8), (16, 24, 4, 24, 4), (64, 72, 4, 64, 0)]
# n, h, w: m = 1 (the m > 1 branch of the variance correction), 2, 70 and a ResNet-like 2 x 56 x 56
SHAPES = [(1, 1, 1), (2, 1, 1), (2, 5, 7)]
BIG = (2, 56, 56)
CASES = [(s, sl) for s in SHAPES for sl in SLICES] + [(BIG, SLICES[1]), (BIG, SLICES[5])]
# the pointwise launches: every C once, m from 1 to the large blob
POINT_CASES = [(SHAPES[0], SLICES[0]), (SHAPES[1], SLICES[2]), (SHAPES[2], SLICES[1]), (SHAPES[2], SLICES[3]), (SHAPES[2], SLICES[4]),
               (BIG, SLICES[1]), (BIG, SLICES[5])]


def stats_allowances(x, eps):
    m = x.shape[0] * x.shape[2] * x.shape[3]
    mean, var = R.batch_stats(x)
    a_mean = ref64.dot_bound_rms(m, np.abs(x.astype(np.float64)).mean(axis=(0, 2, 3))) + 2 * U * np.abs(mean)
    a_var = ref64.dot_bound_rms(m, var) + 4 * U * var + a_mean ** 2
    inv = 1.0 / np.sqrt(var + eps)
    a_inv = 0.5 * inv / (var + eps) * a_var + 3 * U * inv
    return m, mean, var, inv, a_mean, a_var, a_inv


def run_stats(g, x, cs, co, blobs, f, eps):
    n, c, h, w = x.shape
    pix = n * h * w
    nbytes = int(L.load().fcn_batchnorm_workspace_bytes(pix, c))
    assert nbytes >= 2 * 4 * ((c + 3) // 4 * 4)
    xd = g.put(poisoned_nhwc(x, cs, co), at_end=True, name="x")
    outs = []
    for rep in range(2):
        ws = g.put(nbytes, name="workspace run %d" % rep)
        save = g.put(2 * c * 4, at_end=True, name="save run %d" % rep)
        bd = [g.put(b.astype(F32), at_end=True, name="blob %d run %d" % (i, rep)) for i, b in enumerate(blobs)] if blobs is not None else None
        ptrs = [b.ptr for b in bd] if bd else [None, None, None]
        L.call("fcn_batchnorm_stats_f32", xd.ptr, pix, c, cs, co, *ptrs, f, eps, save.ptr, ws.ptr, None)
        L.call("fcn_device_sync")
        outs.append([save.read((2, c))] + ([b.read(blobs[i].shape) for i, b in enumerate(bd)] if bd else []))
    for a, b in zip(*outs):
        assert same_bits(a, b), "two identical calls gave different bits"
    return outs[0]


@pytest.mark.parametrize("shape,sl", CASES)
def test_batch_statistics_and_the_moving_average_step(g, shape, sl):
    (n, h, w), (c, cs, co, _, _) = shape, sl
    rng = np.random.default_rng(31)
    x = (rng.standard_normal((n, c, h, w)) * (1.0 + rng.random((1, c, 1, 1))) + 2.0 * rng.standard_normal((1, c, 1, 1))).astype(F32)
    f, eps = 0.9, 1e-5
    blobs = [rng.standard_normal(c).astype(F32), (rng.random(c) + 0.5).astype(F32), np.array([1.75], F32)]
    m, mean, var, inv, a_mean, a_var, a_inv = stats_allowances(x, eps)
    save, b0, b1, b2 = run_stats(g, x, cs, co, blobs, f, eps)
    assert poison_free(save)
    tag = "m%d c%d" % (m, c)
    within(save[0], mean, a_mean, "mean " + tag)
    within(save[1], inv, a_inv, "invstd " + tag)
    w0, w1, w2 = R.moving_average_step(blobs[0], blobs[1], blobs[2], mean, var, m, f)
    corr = m / (m - 1.0) if m > 1 else 1.0
    within(b0, w0, a_mean + U * (np.abs(blobs[0] * f) + np.abs(w0)), "mean sum " + tag)
    within(b1, w1, a_var * corr + U * (2 * var * corr + np.abs(blobs[1] * f) + np.abs(w1)), "variance sum " + tag)
    within(b2, w2, 2 * U * np.abs(w2), "factor " + tag)
    if m == 1:
        assert np.all(np.abs(b1 - blobs[1] * F32(f)) <= U * np.abs(blobs[1]))      # the variance of one value is zero, uncorrected
    # without the blobs: statistics alone, the same bits in the save area
    assert same_bits(run_stats(g, x, cs, co, None, f, eps)[0], save)


def test_variance_is_centred(g):
    """x with mean about 100 and std about 1: the variance must match float64 within the allowance of a sum of (x - mean)^2 - 2e-5 of the
    variance at m = 6272 - where E[x^2] - E[x]^2 in float32 rounds sums of 1e4 and is off by 1e-3 or more.  The float32 two-pass
    result computed here on the CPU stays inside the same allowance."""
    rng = np.random.default_rng(32)
    n, c, h, w = 2, 16, 56, 56
    x = (100.0 * np.where(rng.random((1, c, 1, 1)) < 0.5, -1.0, 1.0) + rng.standard_normal((n, c, h, w))).astype(F32)
    eps = 1e-5
    m, mean, var, inv, a_mean, a_var, a_inv = stats_allowances(x, eps)
    assert np.all(a_var < 1e-4 * var)
    m32 = x.sum(axis=(0, 2, 3), dtype=F32) / F32(m)
    v32 = ((x - m32.reshape(1, -1, 1, 1)) ** 2).sum(axis=(0, 2, 3), dtype=F32) / F32(m)
    within(v32, var, a_var, "float32 two-pass variance on the CPU")
    naive = (x * x).sum(axis=(0, 2, 3), dtype=F32) / F32(m) - m32 * m32
    assert ref64.worst(naive, var, a_var)[0] > 1.0, "the allowance would let E[x^2] - E[x]^2 through"
    # zero blobs: after one step the variance-sum blob holds var * m / (m - 1), one rounding each for the quotient, the product and the sum
    zeros = [np.zeros(c, F32), np.zeros(c, F32), np.zeros(1, F32)]
    save, b0, b1, b2 = run_stats(g, x, 16, 0, zeros, 0.999, eps)
    corr = m / (m - 1.0)
    within(save[0], mean, a_mean, "mean, |mean| = 100 std")
    within(b1, var * corr, a_var * corr + 3 * U * var * corr, "variance, |mean| = 100 std")
    within(save[1], inv, a_inv, "invstd, |mean| = 100 std")
    assert float(b2[0]) == 1.0 and same_bits(b0, save[0])


def apply_case(rng, shape, c):
    n, h, w = shape
    x = (rng.standard_normal((n, c, h, w)) * 2.0 + rng.standard_normal((1, c, 1, 1))).astype(F32)
    gamma, beta = (rng.standard_normal(c) + 1.5).astype(F32), rng.standard_normal(c).astype(F32)
    return x, gamma, beta


# statistics from: the save area | the three blobs | the blobs with factor == 0 | none (Scale alone); gamma / beta given or NULL
MODES = [("save", True), ("save", False), ("blobs", True), ("blobs", False), ("factor0", True), ("none", True)]


def stats_operands(rng, mode, x, eps):
    """(save array or None, blob arrays or None, mean64, inv64, allowance of xhat) for the operands as the kernel is given them."""
    c = x.shape[1]
    x64 = x.astype(np.float64)
    if mode == "save":
        mean = (x64.mean(axis=(0, 2, 3)) + 0.1 * rng.standard_normal(c)).astype(F32)
        inv = (1.0 / np.sqrt(x64.var(axis=(0, 2, 3)) + 0.5)).astype(F32)
        m64, i64 = mean.astype(np.float64), inv.astype(np.float64)
        return np.stack([mean, inv]), None, m64, i64, 2 * U * np.abs((x64 - ch(m64)) * ch(i64))
    if mode == "none":
        return None, None, None, None, np.zeros(x.shape)
    fac = 0.0 if mode == "factor0" else 3.25
    blobs = [(rng.standard_normal(c) * fac).astype(F32), ((rng.random(c) + 0.5) * fac).astype(F32), np.array([fac], F32)]
    m64, v64 = R.global_stats(*[b.astype(np.float64) for b in blobs])
    i64 = 1.0 / np.sqrt(v64 + eps)
    return None, blobs, m64, i64, U * ch(i64) * (2 * np.abs(ch(m64)) + 6 * np.abs(x64 - ch(m64)))


@pytest.mark.parametrize("mode,scaled", MODES)
@pytest.mark.parametrize("shape,sl", POINT_CASES)
def test_apply(g, shape, sl, mode, scaled):
    (n, h, w), (c, csx, cox, csy, coy) = shape, sl
    rng = np.random.default_rng(33)
    eps = 1e-3
    x, gamma, beta = apply_case(rng, shape, c)
    save, blobs, m64, i64, a_hat = stats_operands(rng, mode, x, eps)
    ga, be = (gamma, beta) if scaled else (None, None)
    pix, c4 = n * h * w, (c + 3) // 4 * 4
    for relu in (0, 1):
        for inplace in (False, True):
            want, hat64, _ = R.chain_fwd(x, m64, None if m64 is None else 1.0 / i64 ** 2 - eps, eps, ga, be, bool(relu))
            g1 = ch(ga if ga is not None else np.ones(c))
            pre = R.chain_fwd(x, m64, None if m64 is None else 1.0 / i64 ** 2 - eps, eps, ga, be, False)[0]      # (ReLU is 1-Lipschitz)
            allow = a_hat * np.abs(g1) + U * (np.abs(hat64 * g1) + np.abs(pre)) + 1e-37
            runs = []
            for rep in range(2):
                xd = g.put(poisoned_nhwc(x, csx, cox), at_end=True, name="x")
                yd = xd if inplace else g.put(poisoned((n, h, w, csy)), at_end=True, name="y")
                ycs, yco = (csx, cox) if inplace else (csy, coy)
                hd = g.put(poisoned((n, h, w, c4)), at_end=True, name="xhat")
                sd = g.put(save, at_end=True, name="save") if save is not None else None
                bd = [g.put(b, at_end=True, name="blob") for b in blobs] if blobs is not None else None
                gd, bed = (g.put(ga, at_end=True, name="gamma"), g.put(be, at_end=True, name="beta")) if scaled else (None, None)
                L.call("fcn_batchnorm_apply_f32", xd.ptr, yd.ptr, hd.ptr, pix, c, csx, cox, ycs, yco, c4, sd.ptr if sd else None,
                       *([b.ptr for b in bd] if bd else [None] * 3), eps, gd.ptr if gd else None, bed.ptr if bed else None, relu, None)
                L.call("fcn_device_sync")
                runs.append((yd.read((n, h, w, ycs)), hd.read((n, h, w, c4))))
            assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]), "two identical calls gave different bits"
            full, hat = runs[0]
            got = nchw(full, c, yco)
            assert poison_free(got) and slice_untouched(full, yco, c) and slice_untouched(hat, 0, c)
            tag = "%s scaled=%d relu=%d inplace=%d m%d c%d" % (mode, scaled, relu, inplace, pix, c)
            within(got, want, allow, "apply " + tag)
            within(nchw(hat, c, 0), hat64, a_hat + 1e-37, "xhat " + tag)
            if mode == "none":
                assert np.array_equal(nchw(hat, c, 0), x)      # Scale alone keeps its input, exactly


# halves: multiples of 8 and one C that is not; a window with poisoned channels on both sides
HALF_SLICES = [(8, 24, 8, 16, 8), (16, 32, 8, 16, 0), (12, 32, 8, 24, 8), (64, 64, 0, 80, 8)]
# odd C (the last half of the window shares its 32-bit word with a pad channel), at the pixel counts of tests/neuron_cases.py's ODD_C:
# (n, h, w) and a slice each
HALF_ODD = [((1, 1, 5), (5, 24, 8, 16, 8)), ((1, 7, 7), (13, 32, 8, 24, 8)), ((1, 1, 5), (7, 24, 8, 16, 0)), ((1, 7, 7), (3, 24, 8, 16, 8))]


@pytest.mark.parametrize("mode", ["blobs", "factor0", "none"])
@pytest.mark.parametrize("c,csx,cox,csy,coy", HALF_SLICES)
def test_apply_half_floats(g, c, csx, cox, csy, coy, mode, shape=(2, 5, 7)):
    rng = np.random.default_rng(34)
    n, h, w = shape
    eps = 1e-3
    x, gamma, beta = apply_case(rng, (n, h, w), c)
    xh = x.astype(np.float16)
    _save, blobs, m64, i64, a_hat = stats_operands(rng, mode, xh.astype(F32), eps)
    pix = n * h * w
    for relu in (0, 1):
        for inplace in (False, True):
            want, hat64, _ = R.chain_fwd(xh.astype(np.float64), m64, None if m64 is None else 1.0 / i64 ** 2 - eps, eps, gamma, beta, bool(relu))
            pre = R.chain_fwd(xh.astype(np.float64), m64, None if m64 is None else 1.0 / i64 ** 2 - eps, eps, gamma, beta, False)[0]
            allow = a_hat * np.abs(ch(gamma)) + U * (np.abs(hat64 * ch(gamma)) + np.abs(pre)) + ref64.U16 * np.abs(pre) + 2.0 ** -24
            runs = []
            for rep in range(2):
                xd = g.put(poisoned_nhwc(xh, csx, cox, dtype=np.float16), at_end=True, name="x")
                yd = xd if inplace else g.put(poisoned((n, h, w, csy), dtype=np.float16), at_end=True, name="y")
                ycs, yco = (csx, cox) if inplace else (csy, coy)
                bd = [g.put(b, at_end=True, name="blob") for b in blobs] if blobs is not None else None
                gd, bed = g.put(gamma, at_end=True, name="gamma"), g.put(beta, at_end=True, name="beta")
                L.call("fcn_batchnorm_apply_f16", xd.ptr, yd.ptr, pix, c, csx, cox, ycs, yco, *([b.ptr for b in bd] if bd else [None] * 3), eps,
                       gd.ptr, bed.ptr, relu, None)
                L.call("fcn_device_sync")
                runs.append(yd.read((n, h, w, ycs), np.float16))
            assert np.array_equal(runs[0].view(np.uint16), runs[1].view(np.uint16)), "two identical calls gave different bits"
            got = nchw(runs[0], c, yco)
            assert poison_free(got) and slice_untouched(runs[0], yco, c)
            within(got, want, allow, "apply f16 %s relu=%d inplace=%d c%d" % (mode, relu, inplace, c))


@pytest.mark.parametrize("mode", ["blobs", "factor0", "none"])
@pytest.mark.parametrize("shape,sl", HALF_ODD)
def test_apply_half_floats_at_odd_widths(g, shape, sl, mode):
    assert sl[0] % 2 == 1
    test_apply_half_floats(g, *sl, mode, shape=shape)


def bwd_case(rng, shape, c, relu):
    n, h, w = shape
    dy = rng.standard_normal((n, c, h, w)).astype(F32)
    xhat = rng.standard_normal((n, c, h, w)).astype(F32)
    y = rng.standard_normal((n, c, h, w)).astype(F32) if relu else None
    return dy, xhat, y


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape,sl", CASES)
def test_backward_reduce(g, shape, sl, relu):
    (n, h, w), (c, csd, cod, csh, coh) = shape, sl
    rng = np.random.default_rng(35)
    dy, xhat, y = bwd_case(rng, shape, c, relu)
    pix = n * h * w
    s1, s2 = R.chain_sums(dy, xhat, y)
    m1, m2 = R.chain_sums(np.abs(dy), np.abs(xhat), y)
    nbytes = int(L.load().fcn_batchnorm_workspace_bytes(pix, c))
    dyd = g.put(poisoned_nhwc(dy, csd, cod), at_end=True, name="dy")
    hd = g.put(poisoned_nhwc(xhat, csh, coh), at_end=True, name="xhat")
    yd = g.put(poisoned_nhwc(y, csd, cod), at_end=True, name="y") if relu else None
    runs = []
    for rep in range(2):
        ws = g.put(nbytes, name="workspace")
        a, b = g.put(c * 4, at_end=True, name="sum dy"), g.put(c * 4, at_end=True, name="sum dy xhat")
        L.call("fcn_batchnorm_bwd_reduce_f32", dyd.ptr, hd.ptr, yd.ptr if yd else None, pix, c, csd, cod, csh, coh, csd, cod, a.ptr, b.ptr,
               ws.ptr, None)
        L.call("fcn_device_sync")
        runs.append((a.read((c,)), b.read((c,))))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]), "two identical calls gave different bits"
    assert poison_free(runs[0][0]) and poison_free(runs[0][1])
    within(runs[0][0], s1, ref64.dot_bound_rms(pix, m1), "sum dy' m%d c%d relu=%d" % (pix, c, relu))
    within(runs[0][1], s2, ref64.dot_bound_rms(pix, m2), "sum dy' xhat m%d c%d relu=%d" % (pix, c, relu))


# invstd from: the save area with the two sums (batch statistics) | the save area without (never planned, but allowed) | the blobs
# (a frozen BatchNorm) | the blobs with factor == 0 | nothing (Scale alone)
BWD_MODES = [("save", True), ("blobs", False), ("factor0", False), ("none", False)]


@pytest.mark.parametrize("mode,centred", BWD_MODES)
@pytest.mark.parametrize("shape,sl", POINT_CASES)
def test_backward_apply(g, shape, sl, mode, centred):
    (n, h, w), (c, csd, cod, csx, cox) = shape, sl
    rng = np.random.default_rng(36)
    eps = 1e-3
    pix, c4 = n * h * w, (c + 3) // 4 * 4
    gamma = (rng.standard_normal(c) + 1.5).astype(F32)
    base = rng.standard_normal((n, c, h, w)).astype(F32)
    for relu in (0, 1):
        dy, xhat, y = bwd_case(rng, shape, c, relu)
        save, blobs, _m64, i64, _ = stats_operands(rng, mode, xhat, eps)
        if i64 is None:
            i64 = np.ones(c)
        kr = 1 if mode in ("save", "none") else 5      # roundings behind gamma * invstd: the product, and the prologue's four for invstd
        s1, s2 = (v.astype(F32) for v in R.chain_sums(dy, xhat, y))      # the sums as the kernel is GIVEN them
        d = R.masked(dy, y)
        k = ch(gamma) * ch(i64)
        if centred:
            a, b = ch(s1.astype(np.float64)) / pix, ch(s2.astype(np.float64)) / pix
            want = k * (d - a - xhat.astype(np.float64) * b)
            allow = U * np.abs(k) * (2 * np.abs(d) + 4 * np.abs(a) + 5 * np.abs(xhat * b)) + U * (2 + kr) * np.abs(want)
        else:
            want = k * d
            allow = U * (1 + kr) * np.abs(want)
        for acc, inplace in ((0, False), (1, False), (0, True)):
            ref = want + base.astype(np.float64) * acc
            runs = []
            for rep in range(2):
                dyd = g.put(poisoned_nhwc(dy, csd, cod), at_end=True, name="dy")
                hd = g.put(poisoned_nhwc(xhat, c4, 0), at_end=True, name="xhat")
                yd = g.put(poisoned_nhwc(y, csd, cod), at_end=True, name="y") if relu else None
                if inplace:
                    dxd, xcs, xco = dyd, csd, cod
                else:
                    dxd, xcs, xco = g.put(poisoned_nhwc(base, csx, cox) if acc else poisoned((n, h, w, csx)), at_end=True, name="dx"), csx, cox
                sd = g.put(save, at_end=True, name="save") if save is not None else None
                bd = [g.put(v, at_end=True, name="blob") for v in blobs] if blobs is not None else None
                gd = g.put(gamma, at_end=True, name="gamma")
                sums = [g.put(s1, at_end=True, name="sum dy"), g.put(s2, at_end=True, name="sum dy xhat")] if centred else None
                L.call("fcn_batchnorm_bwd_apply_f32", dyd.ptr, hd.ptr if centred else None, yd.ptr if yd else None, dxd.ptr, pix, c, csd, cod, c4, 0,
                       csd, cod, xcs, xco, sd.ptr if sd else None, bd[1].ptr if bd else None, bd[2].ptr if bd else None, eps, gd.ptr,
                       sums[0].ptr if sums else None, sums[1].ptr if sums else None, acc, None)
                L.call("fcn_device_sync")
                runs.append(dxd.read((n, h, w, xcs)))
            assert same_bits(runs[0], runs[1]), "two identical calls gave different bits"
            got = nchw(runs[0], c, xco)
            assert poison_free(got) and slice_untouched(runs[0], xco, c)
            within(got, ref, allow + U * np.abs(ref) * acc + 1e-37, "bwd apply %s relu=%d acc=%d inplace=%d m%d c%d" % (mode, relu, acc, inplace, pix, c))


def test_refusals_precede_any_launch(g):
    lib = L.load()
    x = g.put(poisoned((2, 3, 3, 8)), name="x")
    y = g.put(poisoned((2, 3, 3, 8)), name="y")
    ws = g.put(int(lib.fcn_batchnorm_workspace_bytes(18, 8)), name="ws")
    save = g.put(64, name="save")
    assert lib.fcn_batchnorm_workspace_bytes(0, 8) == 0 and lib.fcn_batchnorm_workspace_bytes(18, 0) == 0
    assert lib.fcn_batchnorm_stats_f32(None, 18, 8, 8, 0, None, None, None, 0.9, 1e-5, save.ptr, ws.ptr, None) == 1
    assert lib.fcn_batchnorm_stats_f32(x.ptr, 18, 6, 8, 4, None, None, None, 0.9, 1e-5, save.ptr, ws.ptr, None) == 1      # slice outside the pixel
    assert lib.fcn_batchnorm_stats_f32(x.ptr, 18, 4, 6, 0, None, None, None, 0.9, 1e-5, save.ptr, ws.ptr, None) == 2      # stride of 6 floats
    assert lib.fcn_batchnorm_stats_f32(x.ptr, 18, 4, 8, 0, save.ptr, None, None, 0.9, 1e-5, save.ptr, ws.ptr, None) == 1    # one blob of three
    assert lib.fcn_batchnorm_apply_f32(x.ptr, y.ptr, None, 18, 8, 8, 0, 8, 2, 0, None, None, None, None, 1e-5, None, None, 0, None) == 1
    assert lib.fcn_batchnorm_apply_f32(x.ptr + 4, y.ptr, None, 18, 4, 8, 0, 8, 0, 0, None, None, None, None, 1e-5, None, None, 0, None) == 2
    assert lib.fcn_batchnorm_apply_f16(x.ptr, y.ptr, 18, 8, 12, 0, 16, 0, None, None, None, 1e-5, None, None, 0, None) == 2
    assert lib.fcn_batchnorm_bwd_reduce_f32(x.ptr, y.ptr, None, 18, 8, 8, 0, 8, 0, 0, 0, None, save.ptr, ws.ptr, None) == 1
    assert lib.fcn_batchnorm_bwd_apply_f32(x.ptr, None, None, y.ptr, 18, 8, 8, 0, 0, 0, 0, 0, 8, 0, None, None, None, 1e-5, None, save.ptr, save.ptr,
                                           0, None) == 1      # the sums without xhat
    assert x.unchanged() and y.unchanged() and ws.unchanged() and save.unchanged()
