"""C ABI of the half-float transposed convolution (fcn_tconv2d_prepare_f16 / fcn_tconv2d_f16 / fcn_tconv_bank_pack_f16) and of the
converting crop (fcn_crop_fwd_f16_f32): symbols, the unchanged structs, host-side refusal of bad descriptors and of the other element
type's plan (no GPU: every call here returns before anything touches a device)."""
import ctypes as C
import os
import re

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_tconv2d_num_configs_f16", "fcn_tconv2d_prepare_f16", "fcn_tconv2d_f16", "fcn_tconv_bank_halves", "fcn_tconv_bank_pack_f16",
         "fcn_crop_fwd_f16_f32")
CFG_F16 = 256      # FCN_TCONV_CFG_F16


def _header():
    return open(os.path.join(ROOT, "include", "fcnhip.h")).read()


def test_symbols_are_exported_bound_and_declared():
    lib = L.load()
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
        assert re.search(r"^\s*(?:int|size_t)\s+%s\s*\(" % n, code, flags=re.M), n
    assert L.PROTOTYPES["fcn_tconv2d_prepare_f16"] == L.PROTOTYPES["fcn_tconv2d_prepare"]
    assert L.PROTOTYPES["fcn_tconv2d_f16"] == L.PROTOTYPES["fcn_tconv2d_f32"]
    assert L.PROTOTYPES["fcn_tconv_bank_pack_f16"] == L.PROTOTYPES["fcn_tconv_bank_pack_f32"]
    assert L.PROTOTYPES["fcn_tconv_bank_halves"] == L.PROTOTYPES["fcn_tconv_bank_floats"]
    assert L.PROTOTYPES["fcn_crop_fwd_f16_f32"] == L.PROTOTYPES["fcn_crop_fwd_f16"]
    assert lib.fcn_abi_version() == 2
    assert int(lib.fcn_tconv2d_num_configs_f16()) == 2 and int(lib.fcn_tconv2d_num_configs()) == 1
    assert re.search(r"^#define\s+FCN_TCONV_CFG_F16\s+%d\b" % CFG_F16, code, flags=re.M)


def test_both_structs_are_unchanged():
    assert C.sizeof(L.TConvDesc) == 5 * 8 + 17 * 4 + 4
    assert L.TConvDesc.N.offset == 40 and L.TConvDesc.flags.offset == 40 + 16 * 4
    assert C.sizeof(L.TConvPlan) == 8 + 5 * 4 + 4 and L.TConvPlan.total_tiles.offset == 24


def test_bank_sizes():
    lib = L.load()
    assert int(lib.fcn_tconv_bank_halves(5, 7, 4, 4)) == 16 * 7 * 8 and int(lib.fcn_tconv_bank_halves(21, 21, 16, 16)) == 256 * 21 * 24
    assert int(lib.fcn_tconv_bank_halves(8, 1, 1, 1)) == 8 and int(lib.fcn_tconv_bank_floats(5, 7, 4, 4)) == 16 * 7 * 8
    assert int(lib.fcn_tconv_bank_floats(9, 1, 1, 1)) == 12 and int(lib.fcn_tconv_bank_halves(9, 1, 1, 1)) == 16
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, -1)):
        assert int(lib.fcn_tconv_bank_halves(*bad)) == 0


def _desc(**kw):
    """A consistent k4 s2 pad 1 problem over halves on fake (never dereferenced) 16-byte aligned addresses."""
    d = L.TConvDesc()
    d.a, d.w, d.bias, d.b, d.y2 = 0x10000, 0x20000, 0x30000, 0x40000, None
    d.N, d.H, d.W, d.Ca, d.a_cstride = 1, 7, 9, 3, 8
    d.Cb, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = 6, 4, 4, 1, 2, 14, 18
    d.b_cstride, d.b_coffset, d.y2_cstride, d.y2_coffset, d.flags = 8, 0, 0, 0, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _prepare(d, ws=0x50000, cfg=-1, fn="fcn_tconv2d_prepare_f16"):
    plan = L.TConvPlan()
    rc = getattr(L.load(), fn)(C.byref(d), 1, ws, cfg, C.byref(plan))
    return rc, L.load().fcn_last_error_string().decode()


BAD_ARG = (dict(a=None), dict(w=None), dict(b=None), dict(kh=0), dict(kw=0), dict(stride=0), dict(pad=-1), dict(N=0), dict(H=0), dict(W=-1),
           dict(Ca=0), dict(Cb=0),
           dict(OH=13), dict(OH=16), dict(OW=17), dict(OW=20),              # outside [s (H-1) + k - 2 pad, that + s - 1] = [14..15, 18..19]
           dict(b_cstride=4), dict(b_coffset=4), dict(b_coffset=-1))        # slice wider than the pixel
BAD_ALIGN = (dict(a_cstride=12), dict(a_cstride=4), dict(a_cstride=0), dict(Ca=9),      # no multiple of 8 / below round8(Ca)
             dict(a=0x10008), dict(a=0x10002), dict(w=0x20008), dict(b=0x40001), dict(bias=0x30002),
             dict(flags=L.CONV_OUT_F32, b=0x40002))                          # float32 results need 4 bytes
BAD_UNSUPPORTED = (dict(flags=L.CONV_ACCUM), dict(flags=L.CONV_MASK), dict(flags=L.CONV_SIGMOID2), dict(flags=L.CONV_RELU | L.CONV_ACCUM),
                   dict(flags=L.CONV_MASK, y2=0x60000, y2_cstride=8), dict(y2=0x60000), dict(flags=L.CONV_F16), dict(flags=L.CONV_OUT_F16),
                   dict(stride=65, OH=65 * 6 + 2, OW=65 * 8 + 2), dict(pad=4), dict(pad=5),
                   dict(kh=65, kw=65, pad=0, OH=2 * 6 + 65, OW=2 * 8 + 65),              # more than 4096 taps
                   dict(N=1 << 20, H=64, W=64, OH=128, OW=128))


def test_bad_descriptors_are_refused_on_the_host():
    lib = L.load()
    plan = L.TConvPlan()
    assert lib.fcn_tconv2d_prepare_f16(None, 1, 0x50000, -1, C.byref(plan)) == E_ARG
    assert lib.fcn_tconv2d_prepare_f16(C.byref(_desc()), 0, 0x50000, -1, C.byref(plan)) == E_ARG
    assert lib.fcn_tconv2d_prepare_f16(C.byref(_desc()), -1, 0x50000, -1, C.byref(plan)) == E_ARG
    assert lib.fcn_tconv2d_prepare_f16(C.byref(_desc()), 1, 0x50000, -1, None) == E_ARG
    assert lib.fcn_tconv2d_prepare_f16(C.byref(_desc()), 65536, 0x50000, -1, C.byref(plan)) == E_UNSUPPORTED
    assert _prepare(_desc(), ws=None)[0] == E_ARG                       # valid problem, no workspace
    assert _prepare(_desc(), cfg=int(lib.fcn_tconv2d_num_configs_f16()))[0] == E_ARG
    assert _prepare(_desc(), cfg=-2)[0] == E_ARG
    for cfg in (-1, 0, 1):                                              # both configurations are selectable: refused no earlier than the workspace
        assert _prepare(_desc(), ws=None, cfg=cfg) == (E_ARG, "tconv prepare: null workspace")
    for bad, code in [(b, E_ARG) for b in BAD_ARG] + [(b, E_ALIGN) for b in BAD_ALIGN] + [(b, E_UNSUPPORTED) for b in BAD_UNSUPPORTED]:
        rc, msg = _prepare(_desc(**bad))
        assert rc == code and msg.startswith("tconv"), (bad, rc, msg)
    # the legal flags and what the float32 rules would refuse and the half rules take: refused no earlier than the workspace
    for ok in (dict(b=0x40002), dict(flags=L.CONV_RELU), dict(flags=L.CONV_OUT_F32), dict(flags=L.CONV_RELU | L.CONV_OUT_F32), dict(bias=None),
               dict(OH=15, OW=19), dict(a_cstride=16), dict(b_cstride=7, b_coffset=1)):
        assert _prepare(_desc(**ok), ws=None) == (E_ARG, "tconv prepare: null workspace"), ok


def test_the_float32_prepare_is_as_it_was():
    """Its own rules on the same descriptor: a_cstride in multiples of 4, a 4-byte b, the training flags, no half flag."""
    f32 = dict(fn="fcn_tconv2d_prepare", ws=None)
    for ok in (dict(a_cstride=4), dict(a_cstride=12), dict(flags=L.CONV_ACCUM), dict(flags=L.CONV_MASK, y2=0x60000, y2_cstride=8), dict(y2=0x60000)):
        assert _prepare(_desc(**ok), **f32) == (E_ARG, "tconv prepare: null workspace"), ok
    assert _prepare(_desc(b=0x40002), **f32)[0] == E_ALIGN
    assert _prepare(_desc(a_cstride=6), **f32)[0] == E_ALIGN
    assert _prepare(_desc(), cfg=1, **f32)[0] == E_ARG
    for flag in (L.CONV_F16, L.CONV_OUT_F16, L.CONV_OUT_F32):
        assert _prepare(_desc(flags=flag), **f32)[0] == E_UNSUPPORTED


def _plan(cfg):
    p = L.TConvPlan()
    p.d_probs, p.n, p.cfg, p.grid_x, p.grid_y, p.total_tiles = 0x50000, 1, cfg, 1, 1, 1
    return p


def test_each_launch_refuses_the_other_element_types_plan():
    lib = L.load()
    assert lib.fcn_tconv2d_f16(None, None) == E_ARG
    assert lib.fcn_tconv2d_f16(C.byref(L.TConvPlan()), None) == E_ARG and b"prepare_f16" in lib.fcn_last_error_string()
    assert lib.fcn_tconv2d_f16(C.byref(_plan(0)), None) == E_ARG                    # a plan of fcn_tconv2d_prepare
    assert lib.fcn_tconv2d_f16(C.byref(_plan(CFG_F16 + int(lib.fcn_tconv2d_num_configs_f16()))), None) == E_ARG
    assert lib.fcn_tconv2d_f16(C.byref(_plan(CFG_F16 - 1)), None) == E_ARG
    for cfg in (CFG_F16, CFG_F16 + 1):
        assert lib.fcn_tconv2d_f32(C.byref(_plan(cfg)), None) == E_ARG and b"prepare" in lib.fcn_last_error_string()
    assert lib.fcn_tconv2d_f32(C.byref(L.TConvPlan()), None) == E_ARG


def test_bank_pack_refusals():
    lib = L.load()
    ok = dict(w=0x10000, packed=0x20000, Ca=5, Cb=7, w_cstride=8, kh=4, kw=4)

    def pack(**kw):
        a = dict(ok, **kw)
        return lib.fcn_tconv_bank_pack_f16(a["w"], a["packed"], a["Ca"], a["Cb"], a["w_cstride"], a["kh"], a["kw"], None)
    for bad in (dict(w=None), dict(packed=None), dict(Ca=0), dict(Cb=-1), dict(kh=0), dict(kw=0), dict(w_cstride=6)):
        assert pack(**bad) == E_ARG, bad
        assert lib.fcn_last_error_string().decode().startswith("tconv pack")
    for bad in (dict(w=0x10001), dict(packed=0x20008), dict(packed=0x20002)):
        assert pack(**bad) == E_ALIGN, bad
    assert pack(Ca=1 << 14, Cb=1 << 14, w_cstride=1 << 14) == E_UNSUPPORTED


def test_converting_crop_refusals():
    lib = L.load()
    ok = dict(x=0x10000, y=0x20000, N=2, H=9, W=11, C=5, xcs=8, xco=0, oy=1, ox=2, OH=5, OW=6, ycs=8, yco=0)

    def crop(**kw):
        a = dict(ok, **kw)
        return lib.fcn_crop_fwd_f16_f32(*[a[k] for k in ("x", "y", "N", "H", "W", "C", "xcs", "xco", "oy", "ox", "OH", "OW", "ycs", "yco")], None)
    for bad in (dict(x=None), dict(y=None), dict(N=0), dict(C=0), dict(OH=0), dict(xco=4), dict(yco=4), dict(xco=-1), dict(oy=-1), dict(oy=5),
                dict(ox=6)):
        assert crop(**bad) == E_ARG, bad
        assert lib.fcn_last_error_string().decode().startswith("crop_fwd_f16_f32")
    # x in 16-byte pixels of halves, y in 16-byte pixels of floats
    for bad in (dict(xcs=12), dict(ycs=6), dict(ycs=10, yco=2), dict(x=0x10008), dict(y=0x20004)):
        assert crop(**bad) == E_ALIGN, bad
    assert crop(N=1 << 20, H=64, W=64, OH=64, OW=64, oy=0, ox=0) == E_UNSUPPORTED
