"""C ABI of the depthwise convolution: symbols, descriptor layout, host-side refusal of bad descriptors (no GPU: every call here
returns before anything touches a device)."""
import ctypes as C
import os
import re

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_dwconv2d_num_configs", "fcn_dwconv2d_fwd_f32", "fcn_dwconv2d_fwd_f16", "fcn_dwconv2d_dgrad_f32",
         "fcn_dwconv2d_wgrad_workspace_floats", "fcn_dwconv2d_wgrad_f32")


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
    assert lib.fcn_abi_version() == 2
    assert int(lib.fcn_dwconv2d_num_configs()) >= 2      # one output pixel per lane, and a strip form


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
    fields = _header_fields("fcn_dwconv_desc")
    assert [n for n, _ in fields] == [f[0] for f in L.DwConvDesc._fields_]
    off = 0
    for (n, ptr), (_, ct) in zip(fields, L.DwConvDesc._fields_):
        assert (ct is C.c_void_p) == ptr and getattr(L.DwConvDesc, n).offset == off, n
        off += 8 if ptr else 4
    assert C.sizeof(L.DwConvDesc) == 5 * 8 + 19 * 4 + 4      # (padded to the pointers' alignment)
    # fcn_rconv_desc with C in place of Cin / Cout
    want = [{"Cin": "C"}.get(f[0], f[0]) for f in L.RConvDesc._fields_ if f[0] != "Cout"]
    assert [f[0] for f in L.DwConvDesc._fields_] == want


def test_the_descriptor_helper_applies_caffes_output_rule():
    d = L.dwconv_desc(0x10000, 0x20000, None, 0x40000, 2, 9, 10, 6, 8, 3, 5, 0, 2, 2, 1, 1, 12, 4, L.CONV_RELU)
    assert (d.N, d.H, d.W, d.C, d.x_cstride, d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w) == (2, 9, 10, 6, 8, 3, 5, 0, 2, 2, 1)
    assert (d.OH, d.OW, d.y_cstride, d.y_coffset, d.flags, d.dilation) == (4, 10, 12, 4, L.CONV_RELU, 1)
    d = L.dwconv_desc(0x10000, 0x20000, None, 0x40000, 1, 9, 10, 4, 4, 3, 3, 2, 2, 2, 2, 2, 4, 0)
    assert (d.OH, d.OW, d.dilation) == (5, 5, 2)


def _desc(**kw):
    """A consistent 3x3 pad 1 stride 1 problem over 6 channels on fake (never dereferenced) 16-byte aligned addresses."""
    d = L.DwConvDesc()
    d.x, d.w, d.bias, d.y, d.y2 = 0x10000, 0x20000, 0x30000, 0x40000, None
    d.N, d.H, d.W, d.C, d.x_cstride = 1, 7, 9, 6, 8
    d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.OH, d.OW = 3, 3, 1, 1, 1, 1, 7, 9
    d.y_cstride, d.y_coffset, d.y2_cstride, d.y2_coffset, d.flags, d.dilation = 8, 0, 0, 0, 0, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(name, d, *args):
    rc = getattr(L.load(), name)(C.byref(d), *args)
    return rc, L.load().fcn_last_error_string().decode()


def _fwd(d, cfg=-1):
    return _call("fcn_dwconv2d_fwd_f32", d, cfg, None)


def _f16(d, cfg=-1):
    return _call("fcn_dwconv2d_fwd_f16", d, cfg, None)


def _dgrad(d, cfg=-1):
    return _call("fcn_dwconv2d_dgrad_f32", d, cfg, None)


def _wgrad(d, dw=0x60000, db=0x70000, ws=0x80000, splits=0):
    return _call("fcn_dwconv2d_wgrad_f32", d, dw, db, ws, splits, None)


BAD_ARG = (dict(x=None), dict(y=None), dict(kh=0), dict(kw=0), dict(stride_h=0), dict(stride_w=0), dict(pad_h=-1), dict(pad_w=-1), dict(N=0),
           dict(H=0), dict(W=-1), dict(C=0),
           dict(OH=6), dict(OH=8), dict(OW=8), dict(OW=10),                 # not (H + 2 pad - (dil (k-1) + 1)) / stride + 1 per axis = (7, 9)
           dict(stride_h=2), dict(stride_w=2), dict(pad_h=2), dict(pad_w=0),      # each changes one extent only
           dict(dilation=6, OH=1, OW=1),                                    # the window (13 x 13) exceeds the padded image (9 x 11)
           dict(y_cstride=4), dict(y_coffset=4), dict(y_coffset=-1))        # slice wider than the pixel
BAD_ALIGN = (dict(x_cstride=6), dict(x_cstride=0), dict(x_cstride=4), dict(x=0x10004), dict(y=0x40002))
BAD_UNSUPPORTED = (dict(dilation=0), dict(dilation=-1), dict(N=1 << 20, H=64, W=64, OH=64, OW=64),
                   dict(kh=9, pad_h=4), dict(kw=8, pad_w=4, OW=10))         # more than 7 taps along an axis


def test_forward_and_data_gradient_refuse_on_the_host():
    lib = L.load()
    ncfg = int(lib.fcn_dwconv2d_num_configs())
    for run, allowed in ((_fwd, L.CONV_RELU | L.CONV_ACCUM | L.CONV_MASK), (_dgrad, L.CONV_ACCUM | L.CONV_MASK)):
        name = run.__name__
        assert getattr(lib, {"_fwd": "fcn_dwconv2d_fwd_f32", "_dgrad": "fcn_dwconv2d_dgrad_f32"}[name])(None, -1, None) == E_ARG
        assert run(_desc(), cfg=ncfg)[0] == E_ARG and run(_desc(), cfg=-2)[0] == E_ARG
        for bad in BAD_ARG + (dict(w=None), dict(flags=L.CONV_MASK), dict(flags=L.CONV_MASK, y2=0x60000, y2_cstride=4),
                              dict(flags=L.CONV_MASK, y2=0x60000, y2_cstride=8, y2_coffset=4)):
            rc, msg = run(_desc(**bad))
            assert rc == E_ARG and msg.startswith("dwconv"), (name, bad, rc, msg)
        for bad in BAD_ALIGN + (dict(w=0x20008), dict(bias=0x30002)):
            rc, msg = run(_desc(**bad))
            assert rc == E_ALIGN and msg.startswith("dwconv"), (name, bad, rc, msg)
        others = [f for f in (L.CONV_RELU, L.CONV_SIGMOID2, L.CONV_ACCUM, L.CONV_OUT_F32, L.CONV_F16, L.CONV_OUT_F16, L.CONV_MASK, L.CONV_IMAGE_ONES)
                  if not f & allowed]
        for bad in BAD_UNSUPPORTED + tuple(dict(flags=f) for f in others):
            rc, msg = run(_desc(**bad))
            assert rc == E_UNSUPPORTED and msg.startswith("dwconv"), (name, bad, rc, msg)
    # the strip form: stride_w 1 or 2, no dilation, kw 1 / 3 / 5 / 7 - anything else is refused for configuration 1 alone; forward only
    for bad in (dict(dilation=2, pad_h=2, pad_w=2), dict(stride_w=3, OW=3), dict(kw=2, OW=10), dict(kw=4, pad_w=2, OW=10)):
        rc, msg = _fwd(_desc(**bad), cfg=1)
        assert rc == E_UNSUPPORTED and "strip" in msg, (bad, rc, msg)
    assert _dgrad(_desc(), cfg=1)[0] == E_UNSUPPORTED


def test_the_half_forward_refuses_on_the_host():
    lib = L.load()
    assert lib.fcn_dwconv2d_fwd_f16(None, -1, None) == E_ARG
    for bad in BAD_ARG + (dict(w=None),):
        rc, msg = _f16(_desc(**bad))
        assert rc == E_ARG and msg.startswith("dwconv"), (bad, rc, msg)
    # 8 halves per segment: a stride of 4 or 12 halves splits one, C = 9 needs 16; y as halves is 2-byte aligned, as float32 4-byte
    for bad in (dict(x_cstride=4), dict(x_cstride=12), dict(C=9, y_cstride=16), dict(x=0x10008), dict(y=0x40001), dict(w=0x20008), dict(bias=0x30002),
                dict(y=0x40002, flags=L.CONV_OUT_F32)):
        rc, msg = _f16(_desc(**bad))
        assert rc == E_ALIGN and msg.startswith("dwconv"), (bad, rc, msg)
    for bad in BAD_UNSUPPORTED + (dict(flags=L.CONV_ACCUM), dict(flags=L.CONV_MASK), dict(flags=L.CONV_SIGMOID2), dict(flags=L.CONV_OUT_F16)):
        rc, msg = _f16(_desc(**bad))
        assert rc == E_UNSUPPORTED and msg.startswith("dwconv"), (bad, rc, msg)


def test_the_weight_gradient_refuses_on_the_host():
    lib = L.load()
    assert lib.fcn_dwconv2d_wgrad_f32(None, 0x60000, None, None, 0, None) == E_ARG
    assert _wgrad(_desc(), dw=None)[0] == E_ARG
    for bad in BAD_ARG:
        rc, msg = _wgrad(_desc(**bad))
        assert rc == E_ARG and msg.startswith("dwconv"), (bad, rc, msg)
    for bad in BAD_ALIGN:
        rc, msg = _wgrad(_desc(**bad))
        assert rc == E_ALIGN and msg.startswith("dwconv"), (bad, rc, msg)
    assert _wgrad(_desc(), dw=0x60004)[0] == E_ALIGN and _wgrad(_desc(), db=0x70002)[0] == E_ALIGN
    for bad in BAD_UNSUPPORTED:
        rc, msg = _wgrad(_desc(**bad))
        assert rc == E_UNSUPPORTED and msg.startswith("dwconv"), (bad, rc, msg)
    assert _wgrad(_desc(), splits=-1)[0] == E_ARG and _wgrad(_desc(), splits=1025)[0] == E_ARG and _wgrad(_desc(), splits=64)[0] == E_ARG      # 63 pixels
    # forced splits need the workspace the query sizes: a slab of (kh * kw + 1) * round4(C) floats per split (the taps' rows, then db's)
    slab = (9 + 1) * 8
    assert int(lib.fcn_dwconv2d_wgrad_workspace_floats(C.byref(_desc()), 3)) == 3 * slab
    assert int(lib.fcn_dwconv2d_wgrad_workspace_floats(C.byref(_desc()), 4)) == 4 * slab      # 63 pixels in splits of 16, 16, 16, 15
    assert int(lib.fcn_dwconv2d_wgrad_workspace_floats(C.byref(_desc()), 8)) == 8 * slab
    assert int(lib.fcn_dwconv2d_wgrad_workspace_floats(C.byref(_desc()), 10)) == 9 * slab     # splits of 7 pixels: the tenth would be empty
    assert _wgrad(_desc(), ws=None, splits=3)[0] == E_ARG and _wgrad(_desc(), ws=0x80004, splits=3)[0] == E_ALIGN
    assert int(lib.fcn_dwconv2d_wgrad_workspace_floats(C.byref(_desc()), 0)) == 0       # 63 pixels: the built-in choice is one split
    assert int(lib.fcn_dwconv2d_wgrad_workspace_floats(C.byref(_desc()), 1)) == 0
    big = _desc(N=2, H=33, W=35, OH=33, OW=35)
    floats = int(lib.fcn_dwconv2d_wgrad_workspace_floats(C.byref(big), 0))
    assert floats > 0 and floats % slab == 0 and floats // slab > 1
    assert int(lib.fcn_dwconv2d_wgrad_workspace_floats(C.byref(_desc(dilation=0)), 0)) == 0
    assert int(lib.fcn_dwconv2d_wgrad_workspace_floats(C.byref(_desc()), -1)) == 0
    assert int(lib.fcn_dwconv2d_wgrad_workspace_floats(None, 0)) == 0
