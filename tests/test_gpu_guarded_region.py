"""Guard-banded, poisoned-buffer tests of the region stage's kernels (csrc/region.hip) against tests/ref_region64.py, -m gpu.

Proposal is held to the float64 reference's count, order and batch column exactly, and its corners to 32 float32 ulps of the image's larger
extent: a corner passes through about six roundings and an exp, on boxes the cases keep below twice the image before they are clipped.
ROIPooling is a maximum of inputs and is held to equality, argmax included; PSROIPooling to the allowance of an n-term float32 sum with n
the largest bin, as Normalize's sum is held; the pair softmax to the bound tests/test_gpu_guarded.py uses for the channel softmax.  All
on inputs whose decision margins tests/test_region_ref.py asserts without a GPU - as it asserts which path each Proposal case walks (the
upper half of the sweep's suppressed set, the capacity limits, signed, infinite and NaN scores, an image that is not the map's extent).
Every case is launched twice on the same buffers."""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref_region64 as R
import region_cases as RC
from fcn_object_detector_amd import lib as L
from gpu_util import POISON_WORD, g, launched_twice, poison_free, poisoned, poisoned_nhwc  # noqa: F401  (g is a fixture)

pytestmark = pytest.mark.gpu


def within(y, y64, allow, what=""):
    ratio, at = ref64.worst(y, y64, allow)
    print("BOUND %s %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: element %d is off by %.3g of its allowance" % (what, at, ratio)


def is_poison(a):
    return np.ascontiguousarray(a).view(np.uint32) == POISON_WORD


@pytest.mark.parametrize("name", list(RC.PAIR_SOFTMAX))
def test_pair_softmax(g, name):
    a, cs, co, h, w = RC.PAIR_SOFTMAX[name]
    rng = np.random.default_rng(700 + a)
    x = (rng.random((2, 2 * a, h, w)) * 180 - 90).astype(np.float32)
    x[0, :, 0, 0] = 37.5
    c4 = (2 * a + 3) // 4 * 4
    xd = g.put(poisoned_nhwc(x, cs, co), at_end=True, name="x")
    yd = g.put(poisoned((2, h, w, cs)), name="y")
    out = launched_twice(lambda: L.call("fcn_pair_softmax_f32", xd.ptr, yd.ptr, 2 * h * w, a, cs, co, cs, co, None), lambda: yd.read((2, h, w, cs)))
    y = out[..., co:co + 2 * a].transpose(0, 3, 1, 2)
    want = R.pair_softmax(x)
    assert poison_free(y) and np.all(y[0, :, 0, 0] == 0.5)
    assert np.all(out[..., co + 2 * a:co + c4] == 0), "pad channels of the top are zeros"
    assert np.all(is_poison(out[..., :co])) and np.all(is_poison(out[..., co + c4:]))
    within(y, want, (200 + 2) * ref64.U32 * want + 1e-44, "pair softmax %s" % name)
    assert xd.unchanged()


def proposal_params(c, base, score_cs, score_co, delta_cs, delta_co, rois_cs, rois_co, ts_cs, ts_co):
    par = L.ProposalParams()
    par.H, par.W, par.A, par.feat_stride = c["H"], c["W"], len(base), RC.FEAT_STRIDE
    par.pre_nms_topn, par.post_nms_topn, par.min_size, par.nms_thresh = c["pre"], c["post"], c["min_size"], c["nms"]
    par.score_cstride, par.score_coffset, par.delta_cstride, par.delta_coffset = score_cs, score_co, delta_cs, delta_co
    par.rois_cstride, par.rois_coffset, par.top_score_cstride, par.top_score_coffset = rois_cs, rois_co, ts_cs, ts_co
    for i, v in enumerate(np.asarray(base, np.float32).reshape(-1)):
        par.anchors[i] = v
    return par


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_proposal(g, name, with_scores=True, workspace=None):
    """One case on guard-banded, poisoned buffers of its own, launched twice, held to its reference; `workspace` (a guarded buffer and its
    size) is used as it is, whatever an earlier run left in it, else the case gets a fresh, poisoned one of exactly the size it asks for."""
    lib = L.load()
    c, base, scores, deltas, im_info, ref = RC.proposal_reference(name)
    assert ref["margin"] >= RC.MARGIN      # (tests/test_region_ref.py asserts the same without a GPU)
    a, post = len(base), c["post"]
    s_cs, s_co, d_cs, d_co = 2 * a + 6, 2, 4 * a + 4, 4
    r_cs, r_co = 12, 4
    t_cs, t_co = (8, 4) if with_scores else (0, 0)
    par = proposal_params(c, base, s_cs, s_co, d_cs, d_co, r_cs, r_co, t_cs, t_co)
    nbytes = int(lib.fcn_proposal_workspace_bytes(C.byref(par)))
    assert nbytes > 0
    sd, dd = g.put(poisoned_nhwc(scores, s_cs, s_co), name="scores"), g.put(poisoned_nhwc(deltas, d_cs, d_co), name="deltas")
    imd = g.put(im_info, at_end=True, name="im_info")
    rd, cd = g.put(poisoned((post, r_cs)), name="rois"), g.put(poisoned(1), at_end=True, name="count")
    ws, ws_bytes = workspace or (g.put(nbytes, name="workspace"), nbytes)
    assert ws_bytes >= nbytes
    td = g.put(poisoned((post, t_cs)), name="top scores") if with_scores else None
    rows, top, cnt = launched_twice(
        lambda: L.call("fcn_proposal_f32", sd.ptr, dd.ptr, imd.ptr, C.byref(par), rd.ptr, td.ptr if td else None, cd.ptr, ws.ptr, ws_bytes, None),
        lambda: (rd.read((post, r_cs)), td.read((post, t_cs)) if td else np.zeros(1, np.float32), cd.read((1,), np.int32)))
    k = int(cnt[0])
    print("PROPOSAL %s count %d (reference %d) margin %.3g" % (name, k, ref["count"], ref["margin"]))
    assert k == ref["count"]
    assert sd.unchanged() and dd.unchanged() and imd.unchanged()
    got = rows[:, r_co:r_co + 8]
    assert np.all(is_poison(rows[:, :r_co])) and np.all(is_poison(rows[:, r_co + 8:])), "channels outside the rois' slice were written"
    assert poison_free(got) and np.all(got[k:] == 0) and np.all(got[:, 5:] == 0) and np.all(got[:, 0] == 0), "zero rows, pads and batch column"
    if with_scores:
        ts = top[:, t_co:t_co + 4]
        assert np.all(is_poison(top[:, :t_co])) and np.all(ts[:, 1:] == 0) and np.all(ts[k:] == 0)
        # bit for bit (a -0.0 is not a +0.0 here, an infinity is itself): the rows' scores, hence their order
        assert np.array_equal(bits(ts[:k, 0]), bits(ref["scores"][:k, 0])), "the rows' scores, hence their order"
    if k == 0:
        return
    limit = 32 * float(np.spacing(np.float32(max(im_info[0, 0], im_info[0, 1]))))
    err = float(np.max(np.abs(got[:k, 1:5].astype(np.float64) - ref["rois"][:k, 1:])))
    print("PROPOSAL %s worst |error| %.3g of %.3g" % (name, err, limit))
    assert err <= limit
    # the order, read off the boxes as well: every row is nearer to its own reference row than to any other
    for lo in range(0, k, 512):
        hi = min(lo + 512, k)
        far = np.abs(got[lo:hi, None, 1:5].astype(np.float64) - ref["rois"][None, :k, 1:]).max(axis=2)
        assert np.array_equal(np.argmin(far, axis=1), np.arange(lo, hi))


@pytest.mark.parametrize("name", list(RC.PROPOSALS))
def test_proposal(g, name):
    run_proposal(g, name, with_scores=name != "post_cut")      # (one case without the optional second top)


@pytest.mark.parametrize("name", ["deep_sweep", "signed_scores"])
def test_proposal_without_the_scores_top(g, name):
    """top_scores NULL: the order of the rows is read off the boxes alone."""
    run_proposal(g, name, with_scores=False)


@pytest.mark.parametrize("big_first", [True, False])
def test_proposal_on_a_stale_workspace(g, big_first):
    """One workspace, sized for deep_sweep and never poisoned again, under different problems with their own parameter blocks, as the
    engine reuses one workspace from frame to frame: what a larger problem left in the keys, the slices' counts, the order or the matrix
    must not reach a smaller one (few_survive: 81 places; none_survive: no place at all), nor the other way round."""
    lib = L.load()
    c, base = RC.proposal_inputs("deep_sweep")[:2]
    par = proposal_params(c, base, 2 * len(base) + 6, 2, 4 * len(base) + 4, 4, 12, 4, 8, 4)
    nbytes = int(lib.fcn_proposal_workspace_bytes(C.byref(par)))
    shared = (g.put(nbytes, name="shared workspace"), nbytes)
    names = ["deep_sweep", "few_survive", "none_survive"]
    for name in names if big_first else names[::-1]:
        run_proposal(g, name, workspace=shared)


@pytest.mark.parametrize("with_argmax", [True, False])
@pytest.mark.parametrize("name", list(RC.ROI_POOLS))
def test_roi_pool(g, name, with_argmax):
    n, c, cs, co, ph, pw = RC.ROI_POOLS[name]
    x, want, arg, margin = RC.roi_pool_reference(name)
    assert margin >= RC.MARGIN
    r = len(RC.ROIS)
    c4 = (c + 3) // 4 * 4
    ycs, yo, rcs, ro = c4 + 8, 4, 7, 1
    # huge values around the blob's channels and around the rois: a maximum ignores a NaN
    xd = g.put(poisoned_nhwc(x, cs, co, poison="huge"), at_end=True, poison="huge", name="x")
    wide = poisoned((r, rcs), poison="huge")
    wide[:, ro:ro + 5] = RC.ROIS
    rd = g.put(wide, at_end=True, poison="huge", name="rois")
    yd = g.put(poisoned((r, ph, pw, ycs)), name="y")
    ad = g.put(poisoned((r, ph, pw, c), dtype=np.int32), at_end=True, name="argmax") if with_argmax else None
    out, am = launched_twice(
        lambda: L.call("fcn_roi_pool_fwd_f32", xd.ptr, rd.ptr, yd.ptr, ad.ptr if ad else None, n, RC.POOL_H, RC.POOL_W, c, cs, co, r, rcs, ro, ph, pw,
                       RC.POOL_SCALE, ycs, yo, None),
        lambda: (yd.read((r, ph, pw, ycs)), ad.read((r, ph, pw, c), np.int32) if ad else np.zeros(1, np.int32)))
    y = out[..., yo:yo + c].transpose(0, 3, 1, 2)
    assert np.array_equal(y, want.astype(np.float32)), "a maximum of inputs is exact"
    assert np.all(out[..., yo + c:yo + c4] == 0) and np.all(is_poison(out[..., :yo])) and np.all(is_poison(out[..., yo + c4:]))
    if with_argmax:
        assert np.array_equal(am.transpose(0, 3, 1, 2), arg)
    assert xd.unchanged() and rd.unchanged()


@pytest.mark.parametrize("name", list(RC.PS_POOLS))
def test_psroi_pool(g, name):
    n, od, gs, cs, co = RC.PS_POOLS[name]
    x, want, mag, largest, margin = RC.psroi_pool_reference(name)
    assert margin >= RC.MARGIN
    r = len(RC.PS_ROIS)
    c, c4 = od * gs * gs, (od + 3) // 4 * 4
    ycs, yo, rcs, ro = c4 + 4, 0, 8, 0
    xd = g.put(poisoned_nhwc(x, cs, co), at_end=True, name="x")
    wide = poisoned((r, rcs))
    wide[:, ro:ro + 5] = RC.PS_ROIS
    rd = g.put(wide, name="rois")
    yd = g.put(poisoned((r, gs, gs, ycs)), name="y")
    out = launched_twice(lambda: L.call("fcn_psroi_pool_fwd_f32", xd.ptr, rd.ptr, yd.ptr, n, RC.POOL_H, RC.POOL_W, c, cs, co, r, rcs, ro, od, gs,
                                        RC.PS_SCALE, ycs, yo, None), lambda: yd.read((r, gs, gs, ycs)))
    y = out[..., yo:yo + od].transpose(0, 3, 1, 2)
    assert poison_free(y) and np.all(y[want == 0] == 0)
    assert np.all(out[..., yo + od:yo + c4] == 0) and np.all(is_poison(out[..., yo + c4:]))
    # a sum of at most `largest` terms in float32 (the sqrt(n) allowance of ref64, on the mean of |x|), then one division
    within(y, want, ref64.dot_bound_rms(largest, mag) + 2 * ref64.U32 * np.abs(want), "psroi %s (largest bin %d)" % (name, largest))
    assert xd.unchanged() and rd.unchanged()
