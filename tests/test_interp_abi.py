"""C ABI of the Interp kernels: symbols, prototypes against the header, host-side refusals (no GPU: every call here returns before
anything touches a device)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_interp_fwd_f32", "fcn_interp_fwd_f16", "fcn_interp_bwd_f32")
X, Y = 0x100000, 0x200000      # fake, never dereferenced, 16-byte aligned


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


def fwd(name="fcn_interp_fwd_f32", x=X, y=Y, N=2, H=9, W=11, C_=5, xcs=8, xco=0, pb=-1, pe=-2, OH=12, OW=7, ycs=8, yco=0, out_f32=0):
    tail = (out_f32, None) if name.endswith("f16") else (None,)
    return getattr(L.load(), name)(x, y, N, H, W, C_, xcs, xco, pb, pe, OH, OW, ycs, yco, *tail)


def bwd(dy=Y, dx=X, N=2, H=9, W=11, C_=5, xcs=8, xco=0, pb=-1, pe=-2, OH=12, OW=7, ycs=8, yco=0, acc=0):
    return L.load().fcn_interp_bwd_f32(dy, dx, N, H, W, C_, xcs, xco, pb, pe, OH, OW, ycs, yco, acc, None)


ARG = [dict(x=None), dict(y=None), dict(N=0), dict(H=0), dict(W=0), dict(C_=0), dict(OH=0), dict(OW=0), dict(OH=-3),
       dict(pb=1), dict(pe=1), dict(pb=1, pe=-1),                    # a positive pad
       dict(pb=-4, pe=-5), dict(pb=-9, pe=0), dict(pb=0, pe=-9),     # nothing left of the 9 rows
       dict(xco=4), dict(yco=4), dict(xco=-8), dict(yco=-8)]         # slice wider than the pixel, negative offset


@pytest.mark.parametrize("name", NAMES[:2])
def test_forward_refusals(name):
    for bad in ARG:
        assert fwd(name, **bad) == E_ARG, bad
        assert L.load().fcn_last_error_string().decode().startswith("interp_fwd")
    assert fwd(name, OW=(1 << 24) + 1) == E_UNSUPPORTED and fwd(name, OH=1 << 20, H=1 << 12, pb=0, pe=0) == E_UNSUPPORTED
    assert fwd(name, N=1 << 20, H=1 << 12, pb=0, pe=0) == E_UNSUPPORTED


def test_the_half_form_wants_whole_segments():
    name = "fcn_interp_fwd_f16"
    ok = dict(xcs=16, ycs=16)
    for bad in (dict(xcs=12), dict(xco=4), dict(ycs=20), dict(yco=4), dict(x=X + 8), dict(y=Y + 8)):
        assert fwd(name, **dict(ok, **bad)) == E_ALIGN, bad
    for bad in (dict(ycs=18), dict(yco=2), dict(y=Y + 4), dict(xcs=12)):
        assert fwd(name, out_f32=1, **dict(ok, **bad)) == E_ALIGN, bad
    assert fwd(name, out_f32=2) == E_ARG and fwd(name, out_f32=-1) == E_ARG
    # float32 has a lane-per-element path for such views: no alignment refusal beyond the element's own
    assert fwd("fcn_interp_fwd_f32", x=X + 2) == E_ALIGN and fwd("fcn_interp_fwd_f32", y=Y + 1) == E_ALIGN


def test_backward_refusals():
    for bad in ARG:
        bad = {{"x": "dx", "y": "dy"}.get(k, k): v for k, v in bad.items()}
        assert bwd(**bad) == E_ARG, bad
        assert L.load().fcn_last_error_string().decode().startswith("interp_bwd")
    assert bwd(acc=2) == E_ARG and bwd(acc=-1) == E_ARG
    assert bwd(dx=X + 2) == E_ALIGN and bwd(dy=Y + 3) == E_ALIGN
    assert bwd(OW=(1 << 24) + 1) == E_UNSUPPORTED and bwd(N=1 << 20, H=1 << 12, pb=0, pe=0) == E_UNSUPPORTED
