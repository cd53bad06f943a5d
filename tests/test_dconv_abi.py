"""C ABI of the dilated convolution: symbols, descriptor layout, host-side refusal of bad descriptors (no GPU: every call here
returns before anything touches a device)."""
import ctypes as C
import os
import re

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_dconv2d_num_configs", "fcn_dconv2d_workspace_bytes", "fcn_dconv2d_prepare", "fcn_dconv2d_f32",
         "fcn_dconv2d_wgrad_workspace_floats", "fcn_dconv2d_wgrad_f32")


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
    assert lib.fcn_abi_version() == 1
    assert int(lib.fcn_dconv2d_num_configs()) >= 1


def _header_fields(struct):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fcnhip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ptr = "*" in decl
        names = [n.strip(" *") for n in re.sub(r"^(const\s+)?(float|int32_t|void)\s*\*?", "", decl).split(",")]
        fields += [(n, ptr) for n in names]
    return fields


def test_descriptor_layout_matches_the_header():
    fields = _header_fields("fcn_dconv_desc")
    assert [n for n, _ in fields] == [f[0] for f in L.DConvDesc._fields_]
    off = 0
    for (n, ptr), (_, ct) in zip(fields, L.DConvDesc._fields_):
        assert (ct is C.c_void_p) == ptr and getattr(L.DConvDesc, n).offset == off, n
        off += 8 if ptr else 4
    assert C.sizeof(L.DConvDesc) == 5 * 8 + 18 * 4
    # the fields of fcn_conv_desc without in_shift, plus the dilation
    assert [f[0] for f in L.DConvDesc._fields_] == [f[0] for f in L.ConvDesc._fields_ if f[0] != "in_shift"] + ["dilation"]
    assert [n for n, _ in _header_fields("fcn_dconv_plan")] == [f[0] for f in L.DConvPlan._fields_] == [f[0] for f in L.TConvPlan._fields_]
    assert C.sizeof(L.DConvPlan) == 8 + 5 * 4 + 4 and L.DConvPlan.total_tiles.offset == 24


def _desc(**kw):
    """A consistent k3 d2 p2 s1 problem on fake (never dereferenced) 16-byte aligned addresses."""
    d = L.DConvDesc()
    d.x, d.w, d.bias, d.y, d.y2 = 0x10000, 0x20000, 0x30000, 0x40000, None
    d.N, d.H, d.W, d.Cin, d.x_cstride = 1, 7, 9, 3, 4
    d.Cout, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = 6, 3, 3, 2, 1, 7, 9
    d.y_cstride, d.y_coffset, d.y2_cstride, d.y2_coffset, d.flags, d.dilation = 8, 0, 0, 0, 0, 2
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _prepare(d, ws=0x50000, cfg=-1):
    plan = L.DConvPlan()
    rc = L.load().fcn_dconv2d_prepare(C.byref(d), 1, ws, cfg, C.byref(plan))
    return rc, L.load().fcn_last_error_string().decode()


def _wgrad(d, dw=0x60000, db=0x70000, ws=0x80000):
    rc = L.load().fcn_dconv2d_wgrad_f32(C.byref(d), dw, db, ws, None)
    return rc, L.load().fcn_last_error_string().decode()


BAD_ARG = (dict(x=None), dict(y=None), dict(kh=0), dict(kw=0), dict(stride=0), dict(pad=-1), dict(N=0), dict(H=0), dict(W=-1), dict(Cin=0),
           dict(Cout=0),
           dict(OH=6), dict(OH=8), dict(OW=8), dict(OW=10),                 # not (H + 2 pad - (dil (k-1) + 1)) / stride + 1 = (7, 9)
           dict(dilation=6, OH=1, OW=1),                                    # the dilated window (13) exceeds the padded image (11)
           dict(y_cstride=4), dict(y_coffset=4), dict(y_coffset=-1))        # slice wider than the pixel
BAD_ALIGN = (dict(x_cstride=6), dict(x_cstride=0), dict(Cin=5), dict(x=0x10004), dict(y=0x40002))
BAD_UNSUPPORTED = (dict(dilation=0), dict(dilation=-1), dict(N=1 << 20, H=64, W=64, OH=64, OW=64))


def test_bad_descriptors_are_refused_on_the_host():
    lib = L.load()
    plan = L.DConvPlan()
    assert lib.fcn_dconv2d_prepare(None, 1, 0x50000, -1, C.byref(plan)) == E_ARG
    assert lib.fcn_dconv2d_prepare(C.byref(_desc()), 0, 0x50000, -1, C.byref(plan)) == E_ARG
    assert lib.fcn_dconv2d_prepare(C.byref(_desc()), 1, 0x50000, -1, None) == E_ARG
    assert _prepare(_desc(), ws=None)[0] == E_ARG                       # valid problem, no workspace
    assert _prepare(_desc(), cfg=int(lib.fcn_dconv2d_num_configs()))[0] == E_ARG
    for bad in BAD_ARG + (dict(w=None), dict(flags=L.CONV_MASK), dict(flags=L.CONV_MASK, y2=0x60000, y2_cstride=4)):
        rc, msg = _prepare(_desc(**bad))
        assert rc == E_ARG and msg.startswith("dconv"), (bad, rc, msg)
    for bad in BAD_ALIGN + (dict(w=0x20008),):
        rc, msg = _prepare(_desc(**bad))
        assert rc == E_ALIGN and msg.startswith("dconv"), (bad, rc, msg)
    for bad in BAD_UNSUPPORTED + (dict(flags=L.CONV_SIGMOID2), dict(flags=L.CONV_F16), dict(flags=L.CONV_OUT_F16)):
        rc, msg = _prepare(_desc(**bad))
        assert rc == E_UNSUPPORTED and msg.startswith("dconv"), (bad, rc, msg)
    assert int(lib.fcn_dconv2d_workspace_bytes(C.byref(_desc()), 3)) >= 3 * C.sizeof(L.DConvDesc)
    assert int(lib.fcn_dconv2d_workspace_bytes(C.byref(_desc()), 0)) == 0


def test_the_weight_gradient_refuses_on_the_host():
    lib = L.load()
    assert lib.fcn_dconv2d_wgrad_f32(None, 0x60000, None, None, None) == E_ARG
    assert _wgrad(_desc(), dw=None)[0] == E_ARG
    for bad in BAD_ARG:
        rc, msg = _wgrad(_desc(**bad))
        assert rc == E_ARG and msg.startswith("dconv"), (bad, rc, msg)
    for bad in BAD_ALIGN:
        rc, msg = _wgrad(_desc(**bad))
        assert rc == E_ALIGN and msg.startswith("dconv"), (bad, rc, msg)
    assert _wgrad(_desc(), dw=0x60004)[0] == E_ALIGN
    for bad in BAD_UNSUPPORTED:
        rc, msg = _wgrad(_desc(**bad))
        assert rc == E_UNSUPPORTED and msg.startswith("dconv"), (bad, rc, msg)
    # more than one pixel split (2 x 23 x 25 pixels, nine small tiles) needs the workspace the query sizes
    big = _desc(N=2, H=23, W=25, OH=23, OW=25)
    floats = int(lib.fcn_dconv2d_wgrad_workspace_floats(C.byref(big)))
    assert floats > 0 and floats % (6 * 9 * 4) == 0 and floats // (6 * 9 * 4) > 1
    assert _wgrad(big, ws=None)[0] == E_ARG and _wgrad(big, ws=0x80004)[0] == E_ALIGN
    assert int(lib.fcn_dconv2d_wgrad_workspace_floats(C.byref(_desc()))) == 0       # 63 pixels: one split, no workspace
    assert int(lib.fcn_dconv2d_wgrad_workspace_floats(C.byref(_desc(dilation=0)))) == 0
    assert int(lib.fcn_dconv2d_wgrad_workspace_floats(None)) == 0


def test_the_launch_refuses_an_unprepared_plan():
    lib = L.load()
    assert lib.fcn_dconv2d_f32(None, None) == E_ARG
    assert lib.fcn_dconv2d_f32(C.byref(L.DConvPlan()), None) == E_ARG and b"prepare" in lib.fcn_last_error_string()
