"""Guard-banded, poisoned-buffer parity of the ArgMax kernels against the float64 reference (tests/ref_argmax64.py), -m gpu.

Both element types.  x is a channel window of wider pixels whose other channels hold a HUGE value (3e38, 6e4 for halves): a kernel
that let a pad channel or a neighbouring window into the comparison would report it.  x ends on the last byte in front of its back
red zone, which holds the same huge value: a load past the last pixel's stride would win as well.  y is prefilled with NaN
poison, and every channel outside its window must keep it.  Every case is launched twice and the bits compared.

Checks: indices exact, on the margin cases and on the exact-tie cases of tests/argmax_cases.py.  Values: the plain kernel copies
them (exact); after a blend they lie within dot_bound(6, interpolation of |x|), the threshold of tests/test_gpu_guarded_interp.py for
a float32 result (y is float32 for both element types); probabilities within p * (2 d + (C + 4) 2^-21), d the largest blend bound of
the pixel (it moves numerator and denominator by e^d at most) and (C + 4) 2^-21 for C roundings of the running sum, each with an
expf of an argument below 4 in magnitude (2^-22 from the argument's rounding, 2 ulp from expf) and one rescaling."""
import numpy as np
import pytest

import argmax_cases as A
import ref64
import ref_argmax64 as R
import ref_interp64 as RI
from fcn_object_detector_amd import lib as L
from gpu_util import g, launched_twice, poisoned, poisoned_nhwc, slice_untouched      # noqa: F401  (g: the fixture)

pytestmark = pytest.mark.gpu
E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
FORMS = {"index": 0, "values": L.ARGMAX_VALUES, "pairs": L.ARGMAX_PAIRS}
PLAIN_FN = {False: "fcn_argmax_fwd_f32", True: "fcn_argmax_fwd_f16"}
FUSED_FN = {False: "fcn_interp_argmax_fwd_f32", True: "fcn_interp_argmax_fwd_f16"}


def r4(c):
    return (c + 3) // 4 * 4


def huge_nhwc(x, cstride, coffset, half):
    """NCHW -> the NHWC view at coffset of cstride, every other channel huge and positive."""
    n, c, h, w = x.shape
    out = np.full((n, h, w, cstride), 6e4 if half else 3e38, A.dtype_of(half))
    out[..., coffset:coffset + c] = x.transpose(0, 2, 3, 1)
    return out


def prob_bound(p, c, d=0.0):
    return np.abs(p) * (2.0 * d + (c + 4) * 2.0 ** -21) + 1e-37


def run_plain(g, x, half, top_k, form, soft, xcs, xco, ycs=None, yco=0):
    """Launch twice on guarded buffers -> (indices or None, values or None) as (pixels, k) arrays; the window checks are made here."""
    _, c, _, pixels = x.shape
    outc = 2 * top_k if form == "pairs" else top_k
    ycs = ycs or r4(outc)
    xd = g.put(huge_nhwc(x, xcs, xco, half), at_end=True, poison="huge", name="x")
    yd = g.put(poisoned((pixels, ycs)), name="y")
    flags = FORMS[form] | (L.ARGMAX_SOFTMAX if soft else 0)
    full = launched_twice(lambda: L.call(PLAIN_FN[half], xd.ptr, yd.ptr, pixels, c, xcs, xco, top_k, ycs, yco, flags, None),
                          lambda: yd.read((pixels, ycs)))
    assert slice_untouched(full, yco, outc), "channels of y outside the window were written"
    assert xd.unchanged()
    got = full[:, yco:yco + outc]
    assert np.isfinite(got).all(), "poison (or a huge neighbour) reached y"
    if form == "index":
        return got, None
    if form == "values":
        return None, got
    return got[:, :top_k], got[:, top_k:]


def check_plain(x, top_k, soft, idx, val):
    _, c, _, pixels = x.shape
    x64 = x.astype(np.float64)
    if idx is not None:
        assert np.array_equal(idx, R.argmax(x64, top_k)[0, :, 0, :].T), "indices"
    if val is not None:
        want = R.argmax(x64, top_k, "values", probs=soft)[0, :, 0, :].T
        if soft:
            r, at = ref64.worst(val, want, prob_bound(want, c))
            assert r <= 1.0, (r, at)
        else:
            assert np.array_equal(val.astype(np.float64), want), "the plain kernel reports the values it read"


PLAIN_CASES = [(s, k, form, soft) for s in A.PLAIN_SHAPES for k in A.top_ks(s[0]) for form in FORMS
               for soft in ((False, True) if form != "index" and k in (1, 5) else (False,))]


def plain_id(v):
    s, k, form, soft = v
    return "c%d-k%d-%s%s" % (s[0], k, form, "-softmax" if soft else "")


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("case", PLAIN_CASES, ids=plain_id)
def test_plain_margin_cases(g, case, half):
    (c, cs32, cs16, xco, pixels), top_k, form, soft = case
    x = A.plain_margin(c, pixels, top_k, half)
    idx, val = run_plain(g, x, half, top_k, form, soft, cs16 if half else cs32, xco)
    check_plain(x, top_k, soft, idx, val)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", A.PLAIN_SHAPES, ids=lambda s: "c%d" % s[0])
def test_plain_negative_equal_and_tied_inputs(g, shape, half):
    c, cs32, cs16, xco, pixels = shape
    xcs = cs16 if half else cs32
    for top_k in A.top_ks(c):
        # all negative: an accumulator started at 0 would report 0
        x = A.plain_margin(c, pixels, top_k, half, negative=True)
        check_plain(x, top_k, False, *run_plain(g, x, half, top_k, "pairs", False, xcs, xco))
        # all equal: the ranks read c - 1, c - 2, ...
        x = A.plain_equal(c, pixels, half)
        idx, val = run_plain(g, x, half, top_k, "pairs", False, xcs, xco)
        assert np.array_equal(idx, np.broadcast_to(np.arange(c - 1, c - 1 - top_k, -1), (pixels, top_k))) and (val == -1.5).all()
        # small integers: ties everywhere, decided by the larger index
        x = A.plain_ties(c, pixels, half)
        check_plain(x, top_k, False, *run_plain(g, x, half, top_k, "pairs", False, xcs, xco))


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("top_k,soft", [(1, False), (5, True)])
@pytest.mark.parametrize("shape", A.SWITCH_SHAPES, ids=lambda s: "c%d-p%d" % (s[0], s[4]))
def test_both_sides_of_the_lane_wave_switch(g, shape, top_k, soft, half):
    c, cs32, cs16, xco, pixels = shape
    x = A.plain_margin(c, pixels, top_k, half)
    check_plain(x, top_k, soft, *run_plain(g, x, half, top_k, "pairs", soft, cs16 if half else cs32, xco))


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("form,top_k", [("index", 1), ("index", 2), ("values", 2), ("pairs", 2)])
def test_y_written_into_a_window(g, half, form, top_k):
    c, cs32, cs16, xco, pixels = next(s for s in A.PLAIN_SHAPES if s[0] == 21)
    x = A.plain_margin(c, pixels, top_k, half)
    check_plain(x, top_k, False, *run_plain(g, x, half, top_k, form, False, cs16 if half else cs32, xco, ycs=8, yco=4))


def run_fused(g, x, geom, half, form, soft):
    n, c, h, w, oh, ow, pb, pe = geom
    xcs = (c + 7) // 8 * 8 if half else r4(c)
    outc = 2 if form == "pairs" else 1
    rim = np.full(x.shape, 6e4 if half else 3e38, x.dtype)      # what the pads crop away would win as well
    rim[:, :, -pb:h + pe, -pb:w + pe] = x[:, :, -pb:h + pe, -pb:w + pe]
    xd = g.put(huge_nhwc(rim, xcs, 0, half), at_end=True, poison="huge", name="x")
    yd = g.put(poisoned((n, oh, ow, 4)), name="y")
    flags = FORMS[form] | (L.ARGMAX_SOFTMAX if soft else 0)
    full = launched_twice(lambda: L.call(FUSED_FN[half], xd.ptr, yd.ptr, n, h, w, c, xcs, 0, pb, pe, oh, ow, 4, 0, flags, None),
                          lambda: yd.read((n, oh, ow, 4)))
    assert slice_untouched(full, 0, outc) and xd.unchanged()
    got = full[..., :outc]
    assert np.isfinite(got).all(), "poison (or a huge neighbour) reached y"
    return got


def check_fused(x, geom, form, soft, got):
    n, c, h, w, oh, ow, pb, pe = geom
    x64 = x.astype(np.float64)
    wi = R.interp_argmax(x64, oh, ow, pb, pe)[:, 0]
    wv = R.interp_argmax(x64, oh, ow, pb, pe, "values", probs=soft)[:, 0]
    d = ref64.dot_bound(6, RI.interp_mag(x64, oh, ow, pb, pe))                       # per channel
    if form != "values":
        assert np.array_equal(got[..., 0], wi), "indices"
    if form != "index":
        val = got[..., 1 if form == "pairs" else 0]
        allow = prob_bound(wv, c, d.max(axis=1)) if soft else np.take_along_axis(d, wi[:, None].astype(np.int64), axis=1)[:, 0]
        r, at = ref64.worst(val, wv, allow)
        assert r <= 1.0, (r, at)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("soft", [False, True], ids=["scores", "softmax"])
@pytest.mark.parametrize("form", ["index", "values", "pairs"])
@pytest.mark.parametrize("geom", A.FUSED_GEOMS, ids=lambda v: "-".join(str(a) for a in v))
def test_fused_margin_cases(g, geom, form, soft, half):
    x, _seed = A.fused_margin(*geom, half, soft)
    check_fused(x, geom, form, soft, run_fused(g, x, geom, half, form, soft))


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("soft", [False, True], ids=["scores", "softmax"])
def test_fused_tie_cases(g, soft, half):
    for geom in A.FUSED_GEOMS:
        n, c, h, w = geom[:4]
        x = A.fused_constant_planes(n, c, h, w, half)
        got = run_fused(g, x, geom, half, "pairs", soft)
        assert (got[..., 0] == c - 1).all(), "of equal planes the larger index comes first"
        check_fused(x, geom, "pairs", soft, got)
    geom = A.FUSED_GEOMS[0]
    x = A.fused_integers(*geom[:4], half)
    check_fused(x, geom, "pairs", soft, run_fused(g, x, geom, half, "pairs", soft))


def test_each_contract_error_returns_its_code(g):
    lib = L.load()
    x = np.zeros((1, 8, 5, 6), np.float32)
    xd, yd = g.put(poisoned_nhwc(x, 8, 0), name="x"), g.put(poisoned((1, 9, 11, 8)), name="y")
    for half in (False, True):
        plain, fused = getattr(lib, PLAIN_FN[half]), getattr(lib, FUSED_FN[half])
        p_ok = dict(pixels=30, C=8, xcs=8, xco=0, k=2, ycs=8, yco=0, flags=0)
        f_ok = dict(N=1, H=5, W=6, C=8, xcs=8, xco=0, pb=0, pe=0, OH=9, OW=11, ycs=8, yco=0, flags=0)
        pc = lambda a=xd.ptr, b=yd.ptr, **kw: plain(a, b, *dict(p_ok, **kw).values(), None)
        fc = lambda a=xd.ptr, b=yd.ptr, **kw: fused(a, b, *dict(f_ok, **kw).values(), None)
        for call in (pc, fc):
            assert call(a=None) == E_ARG and call(b=None) == E_ARG
            for bad in (dict(C=0), dict(xco=8), dict(yco=8), dict(flags=16), dict(flags=L.ARGMAX_VALUES | L.ARGMAX_PAIRS)):
                assert call(**bad) == E_ARG, bad
        assert pc(pixels=0) == E_ARG and pc(k=0) == E_ARG and pc(k=9) == E_ARG and pc(k=5, flags=L.ARGMAX_PAIRS) == E_ARG
        assert pc(C=40, xcs=40, k=33, ycs=36) == E_UNSUPPORTED
        assert fc(N=0) == E_ARG and fc(OW=0) == E_ARG and fc(pb=1) == E_ARG and fc(pb=-3, pe=-3) == E_ARG
        assert fc(OW=(1 << 24) + 1) == E_UNSUPPORTED
        if half:
            for bad in (dict(xcs=12), dict(ycs=6), dict(yco=2), dict(a=xd.ptr + 8), dict(b=yd.ptr + 8)):
                assert pc(**bad) == E_ALIGN and fc(**bad) == E_ALIGN, bad
        else:
            assert pc(a=xd.ptr + 2) == E_ALIGN and fc(b=yd.ptr + 1) == E_ALIGN
    L.call("fcn_device_sync")
    assert xd.unchanged() and yd.unchanged()
