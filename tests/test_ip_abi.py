"""C ABI of the InnerProduct kernels: symbols, prototypes against the header, host-side refusals (no GPU: every call here returns
before anything touches a device)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_inner_product_fwd_f32", "fcn_inner_product_fwd_f16", "fcn_inner_product_bwd_data_f32", "fcn_inner_product_bwd_weights_f32")
X, W, B, Y, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000      # fake, never dereferenced, 16-byte aligned
RELU, ACCUM, OUT_F32, NT = 1, 4, 8, 256


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for n in NAMES + ("fcn_inner_product_workspace_bytes", "fcn_inner_product_fwd_workspace_bytes"):
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
    assert lib.fcn_abi_version() == 2


def test_prototypes_match_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fcnhip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+FCN_IP_MAX_ROWS\s+32\b", txt)
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
    assert L.PROTOTYPES["fcn_inner_product_workspace_bytes"] == (C.c_size_t, [C.c_int] * 3)


def test_workspace_query():
    ws = L.load().fcn_inner_product_workspace_bytes
    assert ws(0, 256, 4) == 0 and ws(1, 0, 4) == 0 and ws(1, 256, 0) == 0 and ws(33, 4096, 4096) == 0
    assert ws(1, 4096, 4) > 0                      # GOTURN's fc8-shapes: four outputs fill no chip without a K split
    assert ws(8, 4096, 4) % 16 == 0 and ws(8, 4096, 4) >= ws(1, 4096, 4)
    fwd_ws = L.load().fcn_inner_product_fwd_workspace_bytes
    assert fwd_ws(1, 4096, 4, 3) == 0 and fwd_ws(0, 4096, 4, 4) == 0 and fwd_ws(33, 4096, 4, 4) == 0
    assert fwd_ws(8, 4096, 4, 4) > 0 and fwd_ws(8, 4096, 4, 2) > 0
    # a deploy net holds the forward's partial sums only: CaffeNet fc6 at its batch of 10 needs 0.3 MB, not bwd_data's 10.7 MB of slabs
    assert fwd_ws(10, 9216, 4096, 4) == 2 * 10 * 4096 * 4 and ws(10, 9216, 4096) > 10 * fwd_ws(10, 9216, 4096, 4)
    for m, k, n in ((1, 256, 4), (8, 9216, 1000), (32, 4096, 4096), (10, 4096, 4)):
        assert ws(m, k, n) >= max(fwd_ws(m, k, n, 4), fwd_ws(m, k, n, 2))


def fwd(name="fcn_inner_product_fwd_f32", x=X, xrs=512, w=W, b=B, y=Y, ycs=64, yco=0, M=2, K=512, N=40, flags=0, ws=WS):
    return getattr(L.load(), name)(x, xrs, w, b, y, ycs, yco, M, K, N, flags, ws, None)


def bwd_data(dy=Y, dycs=64, dyco=0, w=W, dx=X, dxrs=512, M=2, K=512, N=40, flags=0, ws=WS):
    return L.load().fcn_inner_product_bwd_data_f32(dy, dycs, dyco, w, dx, dxrs, M, K, N, flags, ws, None)


def bwd_weights(x=X, xrs=512, dy=Y, dycs=64, dyco=0, dw=W, db=B, M=2, K=512, N=40, acc=0):
    return L.load().fcn_inner_product_bwd_weights_f32(x, xrs, dy, dycs, dyco, dw, db, M, K, N, acc, None)


def says(who):
    return L.load().fcn_last_error_string().decode().startswith(who)


@pytest.mark.parametrize("name", NAMES[:2])
def test_forward_refusals(name):
    for bad in (dict(x=None), dict(w=None), dict(y=None), dict(M=0), dict(K=0), dict(N=0), dict(M=-1), dict(xrs=504), dict(yco=-8), dict(yco=32),
                dict(ycs=32), dict(flags=2), dict(flags=64), dict(ws=None, N=4, K=4096, xrs=4096)):
        assert fwd(name, **bad) == E_ARG, bad
        assert says(name[4:]), bad
    if name.endswith("f32"):
        assert fwd(name, flags=OUT_F32) == E_ARG      # float32 has no other output type
    g = 4 if name.endswith("f32") else 8
    for bad in (dict(x=X + 8), dict(w=W + 4), dict(y=Y + 8), dict(b=B + 4), dict(K=512 - g // 2, N=8), dict(xrs=512 + g // 2), dict(ycs=64 + g // 2),
                dict(ws=WS + 8, N=4, K=4096, xrs=4096)):
        assert fwd(name, **bad) == E_ALIGN, bad
        assert says(name[4:]), bad
    assert fwd(name, M=33) == E_UNSUPPORTED and says(name[4:])
    assert fwd(name, N=1 << 16, K=1 << 15, xrs=1 << 15, ycs=1 << 16) == E_UNSUPPORTED
    assert fwd(name, M=32, xrs=1 << 27) == E_UNSUPPORTED


def test_backward_data_refusals():
    who = "inner_product_bwd_data_f32"
    for bad in (dict(dy=None), dict(w=None), dict(dx=None), dict(M=0), dict(K=0), dict(N=0), dict(dxrs=508), dict(dyco=-4), dict(dyco=28),
                dict(flags=1), dict(flags=8), dict(ws=None, K=9216, dxrs=9216, N=4096, dycs=4096)):
        assert bwd_data(**bad) == E_ARG and says(who), bad
    for bad in (dict(dy=Y + 4), dict(w=W + 8), dict(dx=X + 4), dict(K=510), dict(dxrs=514), dict(dycs=66),
                dict(ws=WS + 4, K=9216, dxrs=9216, N=4096, dycs=4096)):
        assert bwd_data(**bad) == E_ALIGN and says(who), bad
    assert bwd_data(M=33) == E_UNSUPPORTED and bwd_data(N=1 << 16, K=1 << 15, dxrs=1 << 15, dycs=1 << 16) == E_UNSUPPORTED
    assert bwd_data(M=32, dycs=1 << 27) == E_UNSUPPORTED


def test_backward_weights_refusals():
    who = "inner_product_bwd_weights_f32"
    for bad in (dict(x=None), dict(dy=None), dict(dw=None), dict(M=0), dict(K=0), dict(N=0), dict(xrs=508), dict(dyco=-4), dict(dyco=28),
                dict(acc=2), dict(acc=-1)):
        assert bwd_weights(**bad) == E_ARG and says(who), bad
    for bad in (dict(x=X + 4), dict(dy=Y + 8), dict(dw=W + 4), dict(db=B + 8), dict(K=510), dict(xrs=514), dict(dycs=66)):
        assert bwd_weights(**bad) == E_ALIGN and says(who), bad
    assert bwd_weights(M=33) == E_UNSUPPORTED and bwd_weights(N=1 << 16, K=1 << 15, xrs=1 << 15, dycs=1 << 16) == E_UNSUPPORTED
