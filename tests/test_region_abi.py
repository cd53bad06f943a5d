"""C ABI of the region stage (csrc/region.hip): symbols, the parameter struct against include/fcnhip.h, host-side refusals (no GPU: every
call here returns before anything touches a device)."""
import ctypes as C
import os
import re

from conftest import ROOT
from fcn_object_detector_amd import lib as L
from fcn_object_detector_amd import region

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_pair_softmax_f32", "fcn_proposal_workspace_bytes", "fcn_proposal_f32", "fcn_roi_pool_fwd_f32", "fcn_psroi_pool_fwd_f32")
X, Y, Z, W = 0x100000, 0x200000, 0x300000, 0x400000      # fake, never dereferenced, 16-byte aligned
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fcnhip.h")).read(), flags=re.S)


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
    assert L.PROTOTYPES["fcn_proposal_workspace_bytes"][0] is C.c_size_t


def test_the_parameter_struct_matches_the_header():
    body = re.search(r"typedef struct fcn_proposal_params \{(.*?)\} fcn_proposal_params;", HEADER, flags=re.S).group(1)
    want = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            kind, names = decl.split(" ", 1)
            want += [(n.strip(), kind) for n in names.split(",")]
    kinds = {"int32_t": C.c_int32, "float": C.c_float}
    got = list(L.ProposalParams._fields_)
    assert [(n, t) for n, t in got[:-1]] == [(n, kinds[k]) for n, k in want[:-1]]
    define = lambda n: int(re.search(r"#define %s (\d+)" % n, HEADER).group(1))
    assert want[-1] == ("anchors[4 * FCN_PROPOSAL_MAX_ANCHORS]", "float") and got[-1][0] == "anchors"
    assert C.sizeof(got[-1][1]) == 16 * define("FCN_PROPOSAL_MAX_ANCHORS") and C.sizeof(L.ProposalParams) == 64 + 16 * define("FCN_PROPOSAL_MAX_ANCHORS")
    limits = (define("FCN_PROPOSAL_MAX_ANCHORS"), define("FCN_PROPOSAL_MAX_CANDIDATES"), define("FCN_PROPOSAL_MAX_PRE_NMS"))
    assert limits == (L.PROPOSAL_MAX_ANCHORS, L.PROPOSAL_MAX_CANDIDATES, L.PROPOSAL_MAX_PRE_NMS) == (region.MAX_ANCHORS, region.MAX_CANDIDATES, region.MAX_PRE_NMS)
    # ResNet-101 R-FCN at 600 x 1000 fits: 9 anchors on a 38 x 63 map, 6000 / 300
    assert 38 * 63 * 9 <= limits[1] and 6000 <= limits[2] and 9 <= limits[0]


def pair(x=X, y=Y, pixels=6, a=5, xcs=12, xo=0, ycs=12, yo=0):
    return L.load().fcn_pair_softmax_f32(x, y, pixels, a, xcs, xo, ycs, yo, None)


def test_pair_softmax_refusals():
    for bad in (dict(x=None), dict(y=None), dict(pixels=0), dict(a=0), dict(xo=-1), dict(xcs=9), dict(ycs=11), dict(yo=1)):      # r4(10) = 12 channels of top
        assert pair(**bad) == E_ARG, bad
        assert L.load().fcn_last_error_string().decode().startswith("pair_softmax")
    assert pair(x=X + 2) == E_ALIGN and pair(y=Y + 1) == E_ALIGN
    assert pair(pixels=1 << 22, xcs=1 << 10, ycs=1 << 10) == E_UNSUPPORTED


def params(**kw):
    d = dict(H=5, W=7, A=9, feat_stride=16, pre_nms_topn=100, post_nms_topn=20, min_size=16.0, nms_thresh=0.7, score_cstride=20, score_coffset=0,
             delta_cstride=36, delta_coffset=0, rois_cstride=8, rois_coffset=0, top_score_cstride=0, top_score_coffset=0)
    d.update(kw)
    p = L.ProposalParams()
    for k, v in d.items():
        setattr(p, k, v)
    return p


def proposal(p, scores=X, deltas=Y, im=Z, rois=W, top=None, count=W + 0x1000, ws=0x800000, ws_bytes=None):
    lib = L.load()
    need = int(lib.fcn_proposal_workspace_bytes(C.byref(p)))
    return lib.fcn_proposal_f32(scores, deltas, im, C.byref(p), rois, top, count, ws, need if ws_bytes is None else ws_bytes, None), need


def test_proposal_refusals():
    lib = L.load()
    assert lib.fcn_proposal_workspace_bytes(None) == 0 and lib.fcn_proposal_workspace_bytes(C.byref(params())) > 0
    for bad in (dict(H=0), dict(W=0), dict(A=0), dict(pre_nms_topn=0), dict(post_nms_topn=0), dict(feat_stride=0), dict(min_size=-1.0),
                dict(nms_thresh=float("nan")), dict(score_cstride=17), dict(delta_cstride=35), dict(score_coffset=4), dict(rois_cstride=7),
                dict(rois_coffset=1), dict(top_score_cstride=3)):
        rc, need = proposal(params(**bad))
        assert (rc, need) == (E_ARG, 0), bad
        assert lib.fcn_last_error_string().decode().startswith("proposal")
    # the capacity limits: anchors, candidates, boxes into the NMS, rows
    for bad in (dict(A=33, score_cstride=68, delta_cstride=132), dict(H=86, W=86), dict(H=38, W=63, pre_nms_topn=6145), dict(post_nms_topn=6145)):
        rc, need = proposal(params(**bad))
        assert (rc, need) == (E_UNSUPPORTED, 0), bad
    assert lib.fcn_proposal_workspace_bytes(C.byref(params(H=38, W=63, pre_nms_topn=6000, post_nms_topn=300))) > 0       # R-FCN at 600 x 1000
    assert lib.fcn_proposal_workspace_bytes(C.byref(params(pre_nms_topn=100000))) > 0      # pre_nms_topn above the 315 candidates: those count
    for bad in (dict(scores=None), dict(deltas=None), dict(im=None), dict(rois=None), dict(count=None), dict(ws=None), dict(ws_bytes=16), dict(top=W + 0x2000)):
        assert proposal(params(), **bad)[0] == E_ARG, bad       # (the last: a scores top without its stride)
    assert proposal(params(), ws=0x800008)[0] == E_ALIGN and proposal(params(), scores=X + 2)[0] == E_ALIGN
    assert proposal(params(), count=W + 0x1001)[0] == E_ALIGN and proposal(params(top_score_cstride=4), top=W + 0x2002)[0] == E_ALIGN


def roi(x=X, rois=Y, y=Z, arg=None, n=2, h=9, w=11, c=5, xcs=8, xo=0, r=8, rcs=8, ro=0, ph=3, pw=2, scale=0.25, ycs=8, yo=0):
    return L.load().fcn_roi_pool_fwd_f32(x, rois, y, arg, n, h, w, c, xcs, xo, r, rcs, ro, ph, pw, scale, ycs, yo, None)


def psroi(x=X, rois=Y, y=Z, n=2, h=9, w=11, c=18, xcs=20, xo=0, r=8, rcs=8, ro=0, od=2, g=3, scale=0.0625, ycs=4, yo=0):
    return L.load().fcn_psroi_pool_fwd_f32(x, rois, y, n, h, w, c, xcs, xo, r, rcs, ro, od, g, scale, ycs, yo, None)


def test_pooling_refusals():
    lib = L.load()
    for bad in (dict(x=None), dict(rois=None), dict(y=None), dict(n=0), dict(h=0), dict(c=0), dict(r=0), dict(ph=0), dict(pw=0), dict(scale=0.0),
                dict(scale=-1.0), dict(scale=float("nan")), dict(xcs=4), dict(xo=4), dict(rcs=4), dict(ro=4), dict(ycs=7), dict(yo=1)):
        assert roi(**bad) == E_ARG, bad
        assert lib.fcn_last_error_string().decode().startswith("roi_pool")
    assert roi(x=X + 2) == E_ALIGN and roi(rois=Y + 1) == E_ALIGN and roi(arg=W + 2) == E_ALIGN
    assert roi(n=1 << 12, h=1 << 10, w=1 << 10) == E_UNSUPPORTED
    for bad in (dict(x=None), dict(r=0), dict(g=0), dict(od=0), dict(scale=0.0), dict(c=17), dict(od=3), dict(g=2), dict(ycs=3), dict(rcs=4)):
        assert psroi(**bad) == E_ARG, bad          # (c = 17, od = 3, g = 2: the bottom does not have output_dim * group_size^2 channels)
        assert lib.fcn_last_error_string().decode().startswith("psroi_pool")
    assert psroi(y=Z + 2) == E_ALIGN
