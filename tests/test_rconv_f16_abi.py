"""C ABI of the half-float rectangular and dilated convolution (fcn_rconv2d_prepare_f16 / fcn_rconv2d_f16): symbols, the unchanged
structs, host-side refusal of bad descriptors and of the other element type's plan (no GPU: every call here returns before anything
touches a device)."""
import ctypes as C
import os
import re

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_rconv2d_num_configs_f16", "fcn_rconv2d_prepare_f16", "fcn_rconv2d_f16")
CFG_F16 = 256      # FCN_RCONV_CFG_F16


def _header():
    return open(os.path.join(ROOT, "include", "fcnhip.h")).read()


def test_symbols_are_exported_bound_and_declared():
    lib = L.load()
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
        assert re.search(r"^\s*int\s+%s\s*\(" % n, code, flags=re.M), n
    assert L.PROTOTYPES["fcn_rconv2d_prepare_f16"] == L.PROTOTYPES["fcn_rconv2d_prepare"]
    assert L.PROTOTYPES["fcn_rconv2d_f16"] == L.PROTOTYPES["fcn_rconv2d_f32"]
    assert lib.fcn_abi_version() == 2
    assert int(lib.fcn_rconv2d_num_configs_f16()) >= 1
    assert re.search(r"^#define\s+FCN_RCONV_CFG_F16\s+%d\b" % CFG_F16, code, flags=re.M)


def test_both_structs_are_unchanged():
    assert C.sizeof(L.RConvDesc) == 5 * 8 + 20 * 4
    assert C.sizeof(L.RConvPlan) == 8 + 5 * 4 + 4 and L.RConvPlan.total_tiles.offset == 24


def _desc(**kw):
    """A consistent 1x7 pad (0, 3) stride 1 problem over halves on fake (never dereferenced) 16-byte aligned addresses."""
    d = L.RConvDesc()
    d.x, d.w, d.bias, d.y, d.y2 = 0x10000, 0x20000, 0x30000, 0x40000, None
    d.N, d.H, d.W, d.Cin, d.x_cstride = 1, 7, 9, 3, 8
    d.Cout, d.kh, d.kw, d.pad_h, d.pad_w, d.stride_h, d.stride_w, d.OH, d.OW = 6, 1, 7, 0, 3, 1, 1, 7, 9
    d.y_cstride, d.y_coffset, d.y2_cstride, d.y2_coffset, d.flags, d.dilation = 8, 0, 0, 0, 0, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _prepare(d, ws=0x50000, cfg=-1):
    plan = L.RConvPlan()
    rc = L.load().fcn_rconv2d_prepare_f16(C.byref(d), 1, ws, cfg, C.byref(plan))
    return rc, L.load().fcn_last_error_string().decode()


BAD_ARG = (dict(x=None), dict(w=None), dict(y=None), dict(kh=0), dict(kw=0), dict(stride_h=0), dict(stride_w=0), dict(pad_h=-1), dict(pad_w=-1),
           dict(N=0), dict(H=0), dict(W=-1), dict(Cin=0), dict(Cout=0),
           dict(OH=6), dict(OH=8), dict(OW=8), dict(OW=10),                 # not (H + 2 pad - (dil (k-1) + 1)) / stride + 1 per axis = (7, 9)
           dict(kh=7, kw=1),                                                # the axes swapped: OH would be 1, OW 15
           dict(dilation=3, OH=7, OW=1),                                    # the window (1 x 19) exceeds the padded image (7 x 15)
           dict(y_cstride=4), dict(y_coffset=4), dict(y_coffset=-1))        # slice wider than the pixel
BAD_ALIGN = (dict(x_cstride=12), dict(x_cstride=4), dict(x_cstride=0), dict(Cin=9),      # no multiple of 8 / below round8(Cin)
             dict(x=0x10008), dict(w=0x20008), dict(y=0x40001), dict(bias=0x30002),
             dict(flags=L.CONV_OUT_F32, y=0x40002))                          # float32 results need 4 bytes
BAD_UNSUPPORTED = (dict(dilation=0), dict(dilation=-1), dict(flags=L.CONV_ACCUM), dict(flags=L.CONV_MASK), dict(flags=L.CONV_SIGMOID2),
                   dict(flags=L.CONV_MASK, y2=0x60000, y2_cstride=8), dict(y2=0x60000), dict(flags=L.CONV_F16), dict(flags=L.CONV_OUT_F16),
                   dict(N=1 << 20, H=64, W=64, OH=64, OW=64),
                   dict(kh=65, kw=65, pad_h=32, pad_w=32, H=64, W=64, OH=64, OW=64))      # more than 4096 taps


def test_bad_descriptors_are_refused_on_the_host():
    lib = L.load()
    plan = L.RConvPlan()
    assert lib.fcn_rconv2d_prepare_f16(None, 1, 0x50000, -1, C.byref(plan)) == E_ARG
    assert lib.fcn_rconv2d_prepare_f16(C.byref(_desc()), 0, 0x50000, -1, C.byref(plan)) == E_ARG
    assert lib.fcn_rconv2d_prepare_f16(C.byref(_desc()), -1, 0x50000, -1, C.byref(plan)) == E_ARG
    assert lib.fcn_rconv2d_prepare_f16(C.byref(_desc()), 1, 0x50000, -1, None) == E_ARG
    assert lib.fcn_rconv2d_prepare_f16(C.byref(_desc()), 65536, 0x50000, -1, C.byref(plan)) == E_UNSUPPORTED
    assert _prepare(_desc(), ws=None)[0] == E_ARG                       # valid problem, no workspace
    assert _prepare(_desc(), ws=0x50008)[0] == E_ALIGN
    assert _prepare(_desc(), cfg=int(lib.fcn_rconv2d_num_configs_f16()))[0] == E_ARG
    assert _prepare(_desc(), cfg=-2)[0] == E_ARG
    for bad, code in [(b, E_ARG) for b in BAD_ARG] + [(b, E_ALIGN) for b in BAD_ALIGN] + [(b, E_UNSUPPORTED) for b in BAD_UNSUPPORTED]:
        rc, msg = _prepare(_desc(**bad))
        assert rc == code and msg.startswith("rconv"), (bad, rc, msg)
    # what the float32 rules would refuse and the half rules take is refused no earlier than the workspace: a 2-byte aligned y
    assert _prepare(_desc(y=0x40002), ws=None) == (E_ARG, _prepare(_desc(), ws=None)[1])


def _plan(cfg):
    p = L.RConvPlan()
    p.d_probs, p.n, p.cfg, p.grid_x, p.grid_y, p.total_tiles = 0x50000, 1, cfg, 1, 1, 1
    return p


def test_each_launch_refuses_the_other_element_types_plan():
    lib = L.load()
    assert lib.fcn_rconv2d_f16(None, None) == E_ARG
    assert lib.fcn_rconv2d_f16(C.byref(L.RConvPlan()), None) == E_ARG and b"prepare_f16" in lib.fcn_last_error_string()
    assert lib.fcn_rconv2d_f16(C.byref(_plan(0)), None) == E_ARG                    # a plan of fcn_rconv2d_prepare
    assert lib.fcn_rconv2d_f16(C.byref(_plan(CFG_F16 + int(lib.fcn_rconv2d_num_configs_f16()))), None) == E_ARG
    assert lib.fcn_rconv2d_f32(C.byref(_plan(CFG_F16)), None) == E_ARG and b"prepare" in lib.fcn_last_error_string()
    assert lib.fcn_rconv2d_f32(C.byref(L.RConvPlan()), None) == E_ARG


def test_the_float32_prepare_still_refuses_half_flags():
    d = _desc(x_cstride=4)
    plan = L.RConvPlan()
    for flag in (L.CONV_F16, L.CONV_OUT_F16, L.CONV_OUT_F32):
        d.flags = flag
        assert L.load().fcn_rconv2d_prepare(C.byref(d), 1, 0x50000, -1, C.byref(plan)) == E_UNSUPPORTED
