"""C ABI of the SSD head (csrc/ssd.hip): symbols, struct layouts against include/fcnhip.h, host-side refusals (no GPU: every call here
returns before anything touches a device)."""
import ctypes as C
import os
import re

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED, E_CAPACITY = 1, 2, 3, 5
NAMES = ("fcn_ssd_gather_f32", "fcn_normalize_fwd_f32", "fcn_detection_output_workspace_bytes", "fcn_detection_output_f32")
X, Y, Z, W = 0x100000, 0x200000, 0x300000, 0x400000      # fake, never dereferenced, 16-byte aligned
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fcnhip.h")).read(), flags=re.S)


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
    assert L.PROTOTYPES["fcn_detection_output_workspace_bytes"][0] is C.c_size_t


def header_struct(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        kind, names = ("ptr", decl.rsplit("*", 1)[1]) if "*" in decl else decl.split(" ", 1)
        fields += [(n.strip(), kind) for n in names.split(",")]
    return fields


def test_struct_layouts_match_the_header():
    kinds = {"ptr": C.c_void_p, "int32_t": C.c_int32, "float": C.c_float}
    for cname, cls in (("fcn_ssd_head", L.SsdHead), ("fcn_detout_params", L.DetOutParams)):
        want = [(n, kinds[k]) for n, k in header_struct(cname)]
        assert [(n, t) for n, t in cls._fields_] == want, cname
    assert C.sizeof(L.SsdHead) == 32 and C.sizeof(L.DetOutParams) == 56
    assert L.SSD_MAX_HEADS == int(re.search(r"#define FCN_SSD_MAX_HEADS (\d+)", HEADER).group(1))
    assert L.DETOUT_MAX_TOPK == int(re.search(r"#define FCN_DETOUT_MAX_TOPK (\d+)", HEADER).group(1))
    assert (L.CODE_CORNER, L.CODE_CENTER_SIZE) == (1, 2)


def heads(*specs):
    arr = (L.SsdHead * len(specs))()
    for h, s in zip(arr, specs):
        d = dict(src=X, pixels=6, C=5, cstride=8, coffset=0, dst_col=0)
        d.update(s)
        for k, v in d.items():
            setattr(h, k, v)
    return arr


def gather(specs=({},), n_heads=None, N=2, dst=Y, rstride=64, cols=60):
    arr = heads(*specs)
    return L.load().fcn_ssd_gather_f32(arr, len(specs) if n_heads is None else n_heads, N, dst, rstride, cols, None)


def test_gather_refusals():
    lib = L.load()
    assert lib.fcn_ssd_gather_f32(None, 1, 2, Y, 64, 60, None) == E_ARG
    for bad in (dict(dst=None), dict(N=0), dict(n_heads=0), dict(cols=0), dict(rstride=59)):
        assert gather(**bad) == E_ARG, bad
        assert lib.fcn_last_error_string().decode().startswith("ssd_gather")
    for bad in (dict(src=None), dict(pixels=0), dict(C=0), dict(coffset=-1), dict(coffset=4), dict(dst_col=-1), dict(dst_col=31), dict(cstride=4)):
        assert gather(specs=(bad,)) == E_ARG, bad
    assert gather(specs=({}, dict(dst_col=29))) == E_ARG                      # columns 0..29 and 29..58 overlap
    assert gather(specs=(dict(src=X + 2),)) == E_ALIGN and gather(dst=Y + 1) == E_ALIGN
    assert gather(specs=tuple({} for _ in range(17))) == E_UNSUPPORTED
    assert gather(N=65536, rstride=64) == E_UNSUPPORTED
    assert gather(specs=(dict(pixels=1 << 20, cstride=1 << 10, C=1),), cols=1 << 21, rstride=1 << 21) == E_UNSUPPORTED


def normalize(x=X, y=Y, s=Z, pixels=4, c=5, xcs=8, xo=0, ycs=8, yo=0, shared=0, eps=1e-10):
    return L.load().fcn_normalize_fwd_f32(x, y, s, pixels, c, xcs, xo, ycs, yo, shared, eps, None)


def test_normalize_refusals():
    for bad in (dict(x=None), dict(y=None), dict(s=None), dict(pixels=0), dict(c=0), dict(shared=2), dict(eps=-1.0), dict(xo=4), dict(yo=-1),
                dict(c=5, ycs=7, xcs=8), dict(yo=4, ycs=11)):                   # the top needs room for r4(C) = 8 channels
        assert normalize(**bad) == E_ARG, bad
        assert L.load().fcn_last_error_string().decode().startswith("normalize")
    assert normalize(x=X + 2) == E_ALIGN and normalize(y=Y + 1) == E_ALIGN and normalize(s=Z + 3) == E_ALIGN
    assert normalize(pixels=1 << 22, xcs=1 << 10, ycs=1 << 10) == E_UNSUPPORTED


def params(**kw):
    d = dict(N=2, P=100, num_classes=5, background=0, code_type=L.CODE_CENTER_SIZE, variance_encoded=0, top_k=20, keep_top_k=10,
             conf_threshold=0.25, nms_threshold=0.45, loc_rstride=400, conf_rstride=500, capacity=20)
    d.update(kw)
    p = L.DetOutParams()
    for k, v in d.items():
        setattr(p, k, v)
    return p


def detout(p, loc=X, conf=Y, priors=Z, rows=W, count=W + 0x1000, ws=0x800000, ws_bytes=None):
    lib = L.load()
    need = int(lib.fcn_detection_output_workspace_bytes(C.byref(p)))
    return lib.fcn_detection_output_f32(loc, conf, priors, C.byref(p), rows, count, ws, need if ws_bytes is None else ws_bytes, None), need


def test_detection_output_refusals():
    lib = L.load()
    assert lib.fcn_detection_output_workspace_bytes(None) == 0 and lib.fcn_detection_output_workspace_bytes(C.byref(params())) > 0
    for bad in (dict(N=0), dict(P=0), dict(num_classes=0), dict(background=5), dict(background=-2), dict(top_k=0), dict(keep_top_k=-3),
                dict(nms_threshold=float("nan")), dict(loc_rstride=399), dict(conf_rstride=499), dict(capacity=-1)):
        rc, need = detout(params(**bad))
        assert (rc, need) == (E_ARG, 0), bad
        assert lib.fcn_last_error_string().decode().startswith("detection_output")
    for bad in (dict(code_type=3), dict(top_k=1025, P=2000, loc_rstride=8000, conf_rstride=10000), dict(top_k=-1, P=1025, loc_rstride=4100, conf_rstride=5125),
                dict(N=70000, capacity=1 << 20), dict(P=1 << 28, num_classes=9, loc_rstride=1 << 30, conf_rstride=1 << 30, N=1)):
        rc, need = detout(params(**bad))
        assert (rc, need) == (E_UNSUPPORTED, 0), bad
    assert detout(params(capacity=19))[0] == E_CAPACITY                                    # 2 images x keep_top_k 10
    assert detout(params(keep_top_k=-1, capacity=159))[0] == E_CAPACITY                    # 2 images x 4 classes x top_k 20
    assert lib.fcn_detection_output_workspace_bytes(C.byref(params(keep_top_k=-1, capacity=160))) > 0
    for bad in (dict(loc=None), dict(conf=None), dict(priors=None), dict(rows=None), dict(count=None), dict(ws=None), dict(ws_bytes=16)):
        assert detout(params(), **bad)[0] == E_ARG, bad
    assert detout(params(), ws=0x800008)[0] == E_ALIGN and detout(params(), loc=X + 2)[0] == E_ALIGN and detout(params(), count=W + 0x1001)[0] == E_ALIGN
