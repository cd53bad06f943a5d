"""C ABI of the Upsample kernels, the half MAX pooling with argmax and the mask read-back: symbols, prototypes against the header,
host-side refusals (no GPU: every call here returns before anything touches a device)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_unpool_fwd_f32", "fcn_unpool_fwd_f16", "fcn_unpool_bwd_f32", "fcn_maxpool_idx_fwd_f16", "fcn_pool_mask_to_nchw_f32")
X, I, Y = 0x100000, 0x200000, 0x300000      # fake, never dereferenced, 16-byte aligned


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
    assert lib.fcn_abi_version() == 2


def test_prototypes_match_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fcnhip.h")).read(), flags=re.S)
    kinds = {"int": C.c_int, "fcn_stream_t": C.c_void_p}
    for n in NAMES:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % n, txt, flags=re.S)
        assert m, n
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            want.append(C.c_void_p if "*" in arg else kinds[arg.rsplit(" ", 1)[0].replace("const ", "")])
        res, args = L.PROTOTYPES[n]
        assert res is C.c_int and list(args) == want, n


# 7 x 9 pooled 2 x 2 / 2 in ceil mode: 4 x 5
def fwd(name="fcn_unpool_fwd_f32", x=X, idx=I, y=Y, N=2, PH=4, PW=5, C_=6, xcs=8, xco=0, k=2, s=2, pad=0, H=7, W=9, ycs=8, yco=0, out_f32=0):
    tail = (out_f32, None) if name.endswith("f16") else (None,)
    return getattr(L.load(), name)(x, idx, y, N, PH, PW, C_, xcs, xco, k, s, pad, H, W, ycs, yco, *tail)


def bwd(dy=Y, idx=I, dx=X, N=2, PH=4, PW=5, C_=6, xcs=8, xco=0, k=2, s=2, pad=0, H=7, W=9, ycs=8, yco=0, acc=0):
    return L.load().fcn_unpool_bwd_f32(dy, idx, dx, N, PH, PW, C_, xcs, xco, k, s, pad, H, W, ycs, yco, acc, None)


ARG = [dict(x=None), dict(idx=None), dict(y=None), dict(N=0), dict(PH=0), dict(PW=-1), dict(C_=0), dict(H=0), dict(W=0), dict(k=0), dict(s=0),
       dict(pad=-1), dict(pad=2),                                      # a pad outside [0, kernel)
       dict(PH=3), dict(PW=4), dict(PH=5), dict(H=9), dict(W=11),      # not the ceil-mode extents: 7 x 9 gives 4 x 5; 9 gives 5, 11 gives 6
       dict(k=3, s=2, pad=1, PH=5),                                    # 3 x 3 / 2 / pad 1 on 7 x 9 is 4 x 5
       dict(xco=4), dict(yco=4), dict(xco=-8), dict(yco=-8)]           # slice wider than the pixel, negative offset


@pytest.mark.parametrize("name", NAMES[:2])
def test_forward_refusals(name):
    ok = dict(xcs=8, ycs=8)
    for bad in ARG:
        assert fwd(name, **dict(ok, **bad)) == E_ARG, bad
        assert L.load().fcn_last_error_string().decode().startswith("unpool_fwd"), bad
    assert fwd(name, k=3, s=2, pad=1, PH=4, PW=5, N=0) == E_ARG
    # views of 2^31 elements or more: y (N * H * W * y_cstride), x, idx
    assert fwd(name, N=1 << 16, H=256, W=256, PH=128, PW=128) == E_UNSUPPORTED
    assert fwd(name, H=1 << 15, W=1 << 16, PH=1 << 14, PW=1 << 15, N=1) == E_UNSUPPORTED


def test_both_extents_that_pool_to_the_same_size_pass_the_geometry_check():
    """8 x 10 pools to 4 x 5 like 7 x 9: the geometry check accepts both.  Shown through a refusal that comes AFTER it (alignment)."""
    assert fwd("fcn_unpool_fwd_f32", H=8, W=10, x=X + 2) == E_ALIGN
    assert fwd("fcn_unpool_fwd_f32", H=7, W=9, x=X + 2) == E_ALIGN
    assert fwd("fcn_unpool_fwd_f32", H=6, W=9, x=X + 2) == E_ARG


def test_alignment_rules():
    # float32: any view of whole floats is served (lane-per-element stores); only a pointer that is no multiple of 4 is refused
    for bad in (dict(x=X + 2), dict(y=Y + 1), dict(idx=I + 2)):
        assert fwd("fcn_unpool_fwd_f32", **bad) == E_ALIGN, bad
    name = "fcn_unpool_fwd_f16"
    ok = dict(xcs=16, ycs=16)
    for bad in (dict(xcs=12), dict(xco=4, C_=4), dict(ycs=20), dict(yco=4, C_=4), dict(x=X + 8), dict(y=Y + 8), dict(idx=I + 2)):
        assert fwd(name, **dict(ok, **bad)) == E_ALIGN, bad
    # a float32 output takes any 4-byte aligned view; the half input keeps its rule
    for bad in (dict(y=Y + 2), dict(xcs=12), dict(x=X + 8)):
        assert fwd(name, out_f32=1, **dict(ok, **bad)) == E_ALIGN, bad
    assert fwd(name, out_f32=2) == E_ARG and fwd(name, out_f32=-1) == E_ARG


def test_backward_refusals():
    for bad in ARG:
        bad = {{"x": "dx", "y": "dy"}.get(k, k): v for k, v in bad.items()}
        assert bwd(**bad) == E_ARG, bad
        assert L.load().fcn_last_error_string().decode().startswith("unpool_bwd")
    assert bwd(acc=2) == E_ARG and bwd(acc=-1) == E_ARG
    assert bwd(dx=X + 2) == E_ALIGN and bwd(dy=Y + 3) == E_ALIGN and bwd(idx=I + 1) == E_ALIGN
    assert bwd(N=1 << 16, H=256, W=256, PH=128, PW=128) == E_UNSUPPORTED


def pool(x=X, y=Y, idx=I, N=2, H=7, W=9, C_=8, xcs=8, k=2, s=2, pad=0, OH=4, OW=5, ycs=8, yco=0):
    return L.load().fcn_maxpool_idx_fwd_f16(x, y, idx, N, H, W, C_, xcs, k, s, pad, OH, OW, ycs, yco, None)


def test_maxpool_idx_f16_refusals():
    for bad in (dict(x=None), dict(y=None), dict(idx=None), dict(N=0), dict(H=0), dict(C_=0), dict(k=0), dict(s=0), dict(pad=2), dict(pad=-1),
                dict(OH=3), dict(OW=6), dict(OH=0), dict(xcs=0), dict(yco=8), dict(yco=-8)):
        assert pool(**bad) == E_ARG, bad
    for bad in (dict(C_=6), dict(C_=4), dict(xcs=12), dict(ycs=12), dict(ycs=24, yco=4), dict(x=X + 8), dict(y=Y + 2), dict(idx=I + 4)):
        assert pool(**bad) == E_ALIGN, bad
    assert pool(N=1 << 16, H=256, W=256, OH=128, OW=128) == E_UNSUPPORTED


def test_mask_read_back_refusals():
    f = L.load().fcn_pool_mask_to_nchw_f32
    assert f(None, Y, 1, 2, 2, 4, None) == E_ARG and f(I, None, 1, 2, 2, 4, None) == E_ARG
    for bad in ((0, 2, 2, 4), (1, 0, 2, 4), (1, 2, -1, 4), (1, 2, 2, 0)):
        assert f(I, Y, *bad, None) == E_ARG, bad
    assert f(I + 2, Y, 1, 2, 2, 4, None) == E_ALIGN and f(I, Y + 1, 1, 2, 2, 4, None) == E_ALIGN
    assert f(I, Y, 1 << 12, 1 << 10, 1 << 9, 4, None) == E_UNSUPPORTED
