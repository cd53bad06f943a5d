"""C ABI of the Crop kernels: symbols, prototypes against the header, host-side refusals (no GPU: every call here returns before
anything touches a device)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_crop_fwd_f32", "fcn_crop_fwd_f16", "fcn_crop_bwd_f32")
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


def fwd(name="fcn_crop_fwd_f32", x=X, y=Y, N=2, H=9, W=11, C_=5, xcs=8, xco=0, oy=2, ox=3, OH=6, OW=7, ycs=8, yco=0):
    return getattr(L.load(), name)(x, y, N, H, W, C_, xcs, xco, oy, ox, OH, OW, ycs, yco, None)


def bwd(dy=Y, dx=X, N=2, H=9, W=11, C_=5, xcs=8, xco=0, oy=2, ox=3, OH=6, OW=7, ycs=8, yco=0, acc=0):
    return L.load().fcn_crop_bwd_f32(dy, dx, N, H, W, C_, xcs, xco, oy, ox, OH, OW, ycs, yco, acc, None)


ARG = [dict(x=None), dict(y=None), dict(N=0), dict(H=0), dict(W=0), dict(C_=0), dict(OH=0), dict(OW=0), dict(oy=-1), dict(ox=-1),
       dict(oy=4), dict(ox=5), dict(OH=8), dict(OW=9),           # off + O > extent, by the offset and by the size
       dict(xco=4), dict(yco=4), dict(xco=-1), dict(yco=-4)]     # slice wider than the pixel


@pytest.mark.parametrize("name", NAMES[:2])
def test_forward_refusals(name):
    for bad in ARG:
        assert fwd(name, **bad) == E_ARG, bad
        assert L.load().fcn_last_error_string().decode().startswith("crop_fwd")
    g = 4 if name.endswith("f32") else 8
    for bad in (dict(xcs=g + g // 2, C_=2), dict(ycs=g + g // 2, C_=2), dict(x=X + 8), dict(y=Y + 4)):
        assert fwd(name, **dict(dict(xcs=2 * g, ycs=2 * g), **bad)) == E_ALIGN, bad
    assert fwd(name, N=1 << 12, H=1 << 10, W=1 << 10, OH=1, OW=1) == E_UNSUPPORTED


def test_backward_refusals():
    for bad in ARG:
        bad = {{"x": "dx", "y": "dy"}.get(k, k): v for k, v in bad.items()}
        assert bwd(**bad) == E_ARG, bad
    assert bwd(acc=2) == E_ARG and bwd(acc=-1) == E_ARG
    for bad in (dict(xcs=6), dict(ycs=10), dict(dx=X + 4), dict(dy=Y + 8)):
        assert bwd(**bad) == E_ALIGN, bad
    assert bwd(N=1 << 12, H=1 << 10, W=1 << 10, OH=1, OW=1) == E_UNSUPPORTED
