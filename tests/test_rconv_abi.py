"""C ABI of the rectangular and dilated convolution: symbols, descriptor layout, host-side refusal of bad descriptors (no GPU: every call here
returns before anything touches a device)."""
import ctypes as C
import os
import re

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_rconv2d_num_configs", "fcn_rconv2d_workspace_bytes", "fcn_rconv2d_prepare", "fcn_rconv2d_f32",
         "fcn_rconv2d_wgrad_workspace_floats", "fcn_rconv2d_wgrad_f32")


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
    assert lib.fcn_abi_version() == 2
    assert int(lib.fcn_rconv2d_num_configs()) >= 1


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
    fields = _header_fields("fcn_rconv_desc")
    assert [n for n, _ in fields] == [f[0] for f in L.RConvDesc._fields_]
    off = 0
    for (n, ptr), (_, ct) in zip(fields, L.RConvDesc._fields_):
        assert (ct is C.c_void_p) == ptr and getattr(L.RConvDesc, n).offset == off, n
        off += 8 if ptr else 4
    assert C.sizeof(L.RConvDesc) == 5 * 8 + 20 * 4
    assert [n for n, _ in _header_fields("fcn_rconv_plan")] == [f[0] for f in L.RConvPlan._fields_]
    assert C.sizeof(L.RConvPlan) == 8 + 5 * 4 + 4 and L.RConvPlan.total_tiles.offset == 24


def test_the_descriptor_is_the_dense_one_per_axis_plus_the_dilation():
    """What the retired fcn_dconv_desc / fcn_dconv_plan promised, of the one descriptor that is left: the fields of fcn_conv_desc without
    in_shift, pad and stride kept per axis, plus the dilation; the plan field for field fcn_tconv_plan."""
    want = []
    for f in L.ConvDesc._fields_:
        want += {"pad": ["pad_h", "pad_w"], "stride": ["stride_h", "stride_w"], "in_shift": []}.get(f[0], [f[0]])
    assert [f[0] for f in L.RConvDesc._fields_] == want + ["dilation"]
    assert [f[0] for f in L.RConvPlan._fields_] == [f[0] for f in L.TConvPlan._fields_]
    assert C.sizeof(L.RConvPlan) == C.sizeof(L.TConvPlan)


def test_the_dilated_symbols_are_gone():
    """ABI version 2: no fcn_dconv* name is exported, bound or declared any more."""
    lib = L.load()
    assert lib.fcn_abi_version() == 2
    for n in NAMES:
        gone = n.replace("rconv", "dconv")
        assert not hasattr(lib, gone) and gone not in L.PROTOTYPES, gone
    assert not [n for n in L.PROTOTYPES if "dconv" in n] and not hasattr(L, "DConvDesc") and not hasattr(L, "DConvPlan")
    assert "dconv" not in open(os.path.join(ROOT, "include", "fcnhip.h")).read()


def _desc(**kw):
    """A consistent 1x7 pad (0, 3) stride 1 problem on fake (never dereferenced) 16-byte aligned addresses."""
    d = L.RConvDesc()
    d.x, d.w, d.bias, d.y, d.y2 = 0x10000, 0x20000, 0x30000, 0x40000, None
    d.N, d.H, d.W, d.Cin, d.x_cstride = 1, 7, 9, 3, 4
    d.Cout, d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.OH, d.OW = 6, 1, 7, 0, 3, 1, 1, 7, 9
    d.y_cstride, d.y_coffset, d.y2_cstride, d.y2_coffset, d.flags, d.dilation = 8, 0, 0, 0, 0, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _square(**kw):
    """A consistent square k3 d2 p2 s1 problem (a dilated layer: equal axes); pad= / stride= set both axes."""
    both = {"pad": ("pad_h", "pad_w"), "stride": ("stride_h", "stride_w")}
    d = _desc(kh=3, kw=3, pad_h=2, pad_w=2, dilation=2)
    for k, v in kw.items():
        for f in both.get(k, (k,)):
            setattr(d, f, v)
    return d


def _prepare(d, ws=0x50000, cfg=-1):
    plan = L.RConvPlan()
    rc = L.load().fcn_rconv2d_prepare(C.byref(d), 1, ws, cfg, C.byref(plan))
    return rc, L.load().fcn_last_error_string().decode()


def _wgrad(d, dw=0x60000, db=0x70000, ws=0x80000):
    rc = L.load().fcn_rconv2d_wgrad_f32(C.byref(d), dw, db, ws, None)
    return rc, L.load().fcn_last_error_string().decode()


BAD_ARG = (dict(x=None), dict(y=None), dict(kh=0), dict(kw=0), dict(stride_h=0), dict(stride_w=0), dict(pad_h=-1), dict(pad_w=-1), dict(N=0),
           dict(H=0), dict(W=-1), dict(Cin=0), dict(Cout=0),
           dict(OH=6), dict(OH=8), dict(OW=8), dict(OW=10),                 # not (H + 2 pad - (dil (k-1) + 1)) / stride + 1 per axis = (7, 9)
           dict(kh=7, kw=1),                                                # the axes swapped: OH would be 1, OW 15
           dict(stride_h=2), dict(stride_w=2), dict(pad_h=1), dict(pad_w=2),      # each changes one extent only
           dict(dilation=3, OH=7, OW=1),                                    # the window (1 x 19) exceeds the padded image (7 x 15)
           dict(y_cstride=4), dict(y_coffset=4), dict(y_coffset=-1))        # slice wider than the pixel
SQUARE_BAD_ARG = (dict(x=None), dict(y=None), dict(kh=0), dict(kw=0), dict(stride=0), dict(pad=-1), dict(N=0), dict(H=0), dict(W=-1), dict(Cin=0),
                  dict(Cout=0),
                  dict(OH=6), dict(OH=8), dict(OW=8), dict(OW=10),          # not (H + 2 pad - (dil (k-1) + 1)) / stride + 1 = (7, 9)
                  dict(dilation=6, OH=1, OW=1),                             # the dilated window (13) exceeds the padded image (11)
                  dict(y_cstride=4), dict(y_coffset=4), dict(y_coffset=-1)) # slice wider than the pixel
SQUARE_BAD_UNSUPPORTED = (dict(dilation=0), dict(dilation=-1), dict(N=1 << 20, H=64, W=64, OH=64, OW=64))
BAD_ALIGN = (dict(x_cstride=6), dict(x_cstride=0), dict(Cin=5), dict(x=0x10004), dict(y=0x40002))
BAD_UNSUPPORTED = (dict(dilation=0), dict(dilation=-1), dict(N=1 << 20, H=64, W=64, OH=64, OW=64),
                   dict(kh=65, kw=65, pad_h=32, pad_w=32, H=64, W=64, OH=64, OW=64))      # more than 4096 taps


def test_good_descriptors_pass_validation():
    """(the size query validates and answers 0 for a refused descriptor: a positive answer means the descriptor was accepted)"""
    lib = L.load()
    big = dict(N=2, H=23, W=25, OH=23, OW=25)
    assert int(lib.fcn_rconv2d_wgrad_workspace_floats(C.byref(_desc(**big)))) > 0
    assert int(lib.fcn_rconv2d_wgrad_workspace_floats(C.byref(_desc(kh=7, kw=1, pad_h=3, pad_w=0, **big)))) > 0
    assert int(lib.fcn_rconv2d_wgrad_workspace_floats(C.byref(_desc(kh=3, kw=5, pad_h=0, pad_w=2, stride_h=2, stride_w=1, N=2, H=23, W=25, OH=11, OW=25)))) > 0
    assert int(lib.fcn_rconv2d_wgrad_workspace_floats(C.byref(_desc(kh=3, kw=3, pad_h=1, pad_w=1, **big)))) > 0      # a square problem is legal


def test_bad_descriptors_are_refused_on_the_host():
    lib = L.load()
    plan = L.RConvPlan()
    assert lib.fcn_rconv2d_prepare(None, 1, 0x50000, -1, C.byref(plan)) == E_ARG
    assert lib.fcn_rconv2d_prepare(C.byref(_desc()), 0, 0x50000, -1, C.byref(plan)) == E_ARG
    assert lib.fcn_rconv2d_prepare(C.byref(_desc()), 1, 0x50000, -1, None) == E_ARG
    assert lib.fcn_rconv2d_prepare(C.byref(_desc()), 65536, 0x50000, -1, C.byref(plan)) == E_UNSUPPORTED
    assert _prepare(_desc(), ws=None)[0] == E_ARG                       # valid problem, no workspace
    assert _prepare(_desc(), cfg=int(lib.fcn_rconv2d_num_configs()))[0] == E_ARG
    assert _prepare(_desc(), cfg=-2)[0] == E_ARG
    for bad in BAD_ARG + (dict(w=None), dict(flags=L.CONV_MASK), dict(flags=L.CONV_MASK, y2=0x60000, y2_cstride=4)):
        rc, msg = _prepare(_desc(**bad))
        assert rc == E_ARG and msg.startswith("rconv"), (bad, rc, msg)
    for bad in BAD_ALIGN + (dict(w=0x20008), dict(bias=0x30002)):
        rc, msg = _prepare(_desc(**bad))
        assert rc == E_ALIGN and msg.startswith("rconv"), (bad, rc, msg)
    for bad in BAD_UNSUPPORTED + (dict(flags=L.CONV_SIGMOID2), dict(flags=L.CONV_F16), dict(flags=L.CONV_OUT_F16)):
        rc, msg = _prepare(_desc(**bad))
        assert rc == E_UNSUPPORTED and msg.startswith("rconv"), (bad, rc, msg)
    assert int(lib.fcn_rconv2d_workspace_bytes(C.byref(_desc()), 3)) >= 3 * C.sizeof(L.RConvDesc)
    assert int(lib.fcn_rconv2d_workspace_bytes(C.byref(_desc()), 0)) == 0


def test_bad_square_dilated_descriptors_are_refused_on_the_host():
    assert int(L.load().fcn_rconv2d_wgrad_workspace_floats(C.byref(_square(N=2, H=23, W=25, OH=23, OW=25)))) > 0      # the problem itself is accepted
    for bad in SQUARE_BAD_ARG + (dict(w=None), dict(flags=L.CONV_MASK), dict(flags=L.CONV_MASK, y2=0x60000, y2_cstride=4)):
        rc, msg = _prepare(_square(**bad))
        assert rc == E_ARG and msg.startswith("rconv"), (bad, rc, msg)
    for bad in BAD_ALIGN + (dict(w=0x20008),):
        rc, msg = _prepare(_square(**bad))
        assert rc == E_ALIGN and msg.startswith("rconv"), (bad, rc, msg)
    for bad in SQUARE_BAD_UNSUPPORTED + (dict(flags=L.CONV_SIGMOID2), dict(flags=L.CONV_F16), dict(flags=L.CONV_OUT_F16)):
        rc, msg = _prepare(_square(**bad))
        assert rc == E_UNSUPPORTED and msg.startswith("rconv"), (bad, rc, msg)


def test_the_weight_gradient_refuses_square_dilated_problems_on_the_host():
    lib = L.load()
    assert _wgrad(_square(), dw=None)[0] == E_ARG
    for bad in SQUARE_BAD_ARG:
        rc, msg = _wgrad(_square(**bad))
        assert rc == E_ARG and msg.startswith("rconv"), (bad, rc, msg)
    for bad in BAD_ALIGN:
        rc, msg = _wgrad(_square(**bad))
        assert rc == E_ALIGN and msg.startswith("rconv"), (bad, rc, msg)
    assert _wgrad(_square(), dw=0x60004)[0] == E_ALIGN
    for bad in SQUARE_BAD_UNSUPPORTED:
        rc, msg = _wgrad(_square(**bad))
        assert rc == E_UNSUPPORTED and msg.startswith("rconv"), (bad, rc, msg)
    # more than one pixel split (2 x 23 x 25 pixels, nine small tiles) needs the workspace the query sizes
    big = _square(N=2, H=23, W=25, OH=23, OW=25)
    floats = int(lib.fcn_rconv2d_wgrad_workspace_floats(C.byref(big)))
    assert floats > 0 and floats % (6 * 9 * 4) == 0 and floats // (6 * 9 * 4) > 1
    assert _wgrad(big, ws=None)[0] == E_ARG and _wgrad(big, ws=0x80004)[0] == E_ALIGN
    assert int(lib.fcn_rconv2d_wgrad_workspace_floats(C.byref(_square()))) == 0       # 63 pixels: one split, no workspace
    assert int(lib.fcn_rconv2d_wgrad_workspace_floats(C.byref(_square(dilation=0)))) == 0


def test_the_weight_gradient_refuses_on_the_host():
    lib = L.load()
    assert lib.fcn_rconv2d_wgrad_f32(None, 0x60000, None, None, None) == E_ARG
    assert _wgrad(_desc(), dw=None)[0] == E_ARG
    for bad in BAD_ARG:
        rc, msg = _wgrad(_desc(**bad))
        assert rc == E_ARG and msg.startswith("rconv"), (bad, rc, msg)
    for bad in BAD_ALIGN:
        rc, msg = _wgrad(_desc(**bad))
        assert rc == E_ALIGN and msg.startswith("rconv"), (bad, rc, msg)
    assert _wgrad(_desc(), dw=0x60004)[0] == E_ALIGN and _wgrad(_desc(), db=0x70002)[0] == E_ALIGN
    for bad in BAD_UNSUPPORTED:
        rc, msg = _wgrad(_desc(**bad))
        assert rc == E_UNSUPPORTED and msg.startswith("rconv"), (bad, rc, msg)
    # more than one pixel split (2 x 23 x 25 pixels, seven small tiles) needs the workspace the query sizes
    big = _desc(N=2, H=23, W=25, OH=23, OW=25)
    floats = int(lib.fcn_rconv2d_wgrad_workspace_floats(C.byref(big)))
    assert floats > 0 and floats % (6 * 7 * 4) == 0 and floats // (6 * 7 * 4) > 1
    assert _wgrad(big, ws=None)[0] == E_ARG and _wgrad(big, ws=0x80004)[0] == E_ALIGN
    assert int(lib.fcn_rconv2d_wgrad_workspace_floats(C.byref(_desc()))) == 0       # 63 pixels: one split, no workspace
    assert int(lib.fcn_rconv2d_wgrad_workspace_floats(C.byref(_desc(dilation=0)))) == 0
    assert int(lib.fcn_rconv2d_wgrad_workspace_floats(None)) == 0


def test_the_launch_refuses_an_unprepared_plan():
    lib = L.load()
    assert lib.fcn_rconv2d_f32(None, None) == E_ARG
    assert lib.fcn_rconv2d_f32(C.byref(L.RConvPlan()), None) == E_ARG and b"prepare" in lib.fcn_last_error_string()
