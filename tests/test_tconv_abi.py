"""C ABI of the transposed convolution: symbols, descriptor layout, host-side refusal of bad descriptors (no GPU: every call here
returns before anything touches a device)."""
import ctypes as C
import os
import re

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_tconv2d_num_configs", "fcn_tconv2d_workspace_bytes", "fcn_tconv2d_prepare", "fcn_tconv2d_f32", "fcn_tconv_bank_floats",
         "fcn_tconv_bank_pack_f32", "fcn_channel_sum_f32")


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
    assert lib.fcn_abi_version() == 2
    assert int(lib.fcn_tconv2d_num_configs()) >= 1


def test_descriptor_layout_matches_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fcnhip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct fcn_tconv_desc \{(.*?)\} fcn_tconv_desc;", txt, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ptr = "*" in decl
        names = [n.strip(" *") for n in re.sub(r"^(const\s+)?(float|int32_t)\s*\*?", "", decl).split(",")]
        fields += [(n, ptr) for n in names]
    assert [n for n, _ in fields] == [f[0] for f in L.TConvDesc._fields_]
    off = 0
    for (n, ptr), (_, ct) in zip(fields, L.TConvDesc._fields_):
        assert (ct is C.c_void_p) == ptr and getattr(L.TConvDesc, n).offset == off, n
        off += 8 if ptr else 4
    assert C.sizeof(L.TConvDesc) == 5 * 8 + 17 * 4 + 4      # (tail padding to the pointers' alignment)
    assert C.sizeof(L.TConvPlan) == 8 + 5 * 4 + 4 and L.TConvPlan.total_tiles.offset == 24


def _desc(**kw):
    """A consistent k4 s2 p1 problem on fake (never dereferenced) 16-byte aligned addresses."""
    d = L.TConvDesc()
    d.a, d.w, d.bias, d.b, d.y2 = 0x10000, 0x20000, 0x30000, 0x40000, None
    d.N, d.H, d.W, d.Ca, d.a_cstride = 1, 5, 7, 3, 4
    d.Cb, d.kh, d.kw, d.pad, d.stride, d.OH, d.OW = 6, 4, 4, 1, 2, 10, 14
    d.b_cstride, d.b_coffset, d.y2_cstride, d.y2_coffset, d.flags = 8, 0, 0, 0, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _prepare(d, ws=0x50000, cfg=-1):
    plan = L.TConvPlan()
    rc = L.load().fcn_tconv2d_prepare(C.byref(d), 1, ws, cfg, C.byref(plan))
    return rc, L.load().fcn_last_error_string().decode()


def test_bad_descriptors_are_refused_on_the_host():
    lib = L.load()
    plan = L.TConvPlan()
    assert lib.fcn_tconv2d_prepare(None, 1, 0x50000, -1, C.byref(plan)) == E_ARG
    assert lib.fcn_tconv2d_prepare(C.byref(_desc()), 0, 0x50000, -1, C.byref(plan)) == E_ARG
    assert lib.fcn_tconv2d_prepare(C.byref(_desc()), 1, 0x50000, -1, None) == E_ARG
    assert _prepare(_desc(), ws=None)[0] == E_ARG                       # valid problem, no workspace
    assert _prepare(_desc(), cfg=int(lib.fcn_tconv2d_num_configs()))[0] == E_ARG
    for bad in (dict(a=None), dict(w=None), dict(b=None), dict(kh=0), dict(kw=0), dict(stride=0), dict(pad=-1), dict(N=0), dict(Ca=0), dict(Cb=0),
                dict(OH=9), dict(OH=12), dict(OW=13), dict(OW=16),               # outside [s(H-1)+k-2p, +s-1] = [10..11, 14..15]
                dict(b_cstride=4), dict(b_coffset=4), dict(b_coffset=-1),        # slice wider than the pixel
                dict(flags=L.CONV_MASK), dict(flags=L.CONV_MASK, y2=0x60000, y2_cstride=4)):
        rc, msg = _prepare(_desc(**bad))
        assert rc == E_ARG and msg.startswith("tconv"), (bad, rc, msg)
    for bad in (dict(a_cstride=6), dict(a_cstride=0), dict(Ca=5), dict(a=0x10004), dict(w=0x20008), dict(b=0x40002)):
        rc, msg = _prepare(_desc(**bad))
        assert rc == E_ALIGN, (bad, rc, msg)
    for bad in (dict(stride=65, OH=65 * 4 + 2, OW=65 * 6 + 2), dict(pad=4, OH=4, OW=8), dict(flags=L.CONV_SIGMOID2), dict(flags=L.CONV_F16),
                dict(N=1 << 20, H=64, W=64, OH=128, OW=128)):
        rc, msg = _prepare(_desc(**bad))
        assert rc == E_UNSUPPORTED, (bad, rc, msg)
    # legal: the two output sizes of the range, in both axes
    assert int(lib.fcn_tconv2d_workspace_bytes(C.byref(_desc()), 3)) >= 3 * C.sizeof(L.TConvDesc)
    assert int(lib.fcn_tconv2d_workspace_bytes(C.byref(_desc()), 0)) == 0


def test_launch_and_helpers_refuse_without_a_device():
    lib = L.load()
    assert lib.fcn_tconv2d_f32(None, None) == E_ARG
    assert lib.fcn_tconv2d_f32(C.byref(L.TConvPlan()), None) == E_ARG and b"prepare" in lib.fcn_last_error_string()
    assert int(lib.fcn_tconv_bank_floats(5, 3, 2, 3)) == 2 * 3 * 3 * 8 and int(lib.fcn_tconv_bank_floats(0, 3, 2, 3)) == 0
    assert lib.fcn_tconv_bank_pack_f32(None, 0x1000, 4, 4, 4, 3, 3, None) == E_ARG
    assert lib.fcn_tconv_bank_pack_f32(0x1000, 0x2000, 4, 5, 4, 3, 3, None) == E_ARG        # w_cstride below Cb
    assert lib.fcn_tconv_bank_pack_f32(0x1000, 0x2004, 4, 4, 4, 3, 3, None) == E_ALIGN
    assert lib.fcn_channel_sum_f32(None, 0x1000, 4, 4, 4, 0, None) == E_ARG
    assert lib.fcn_channel_sum_f32(0x1000, 0x2000, 4, 4, 4, 1, None) == E_ARG               # slice wider than the pixel
    assert lib.fcn_channel_sum_f32(0x1000, 0x2000, 0, 4, 4, 0, None) == E_ARG
    assert lib.fcn_channel_sum_f32(0x1002, 0x2000, 4, 4, 4, 0, None) == E_ALIGN
