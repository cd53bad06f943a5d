"""C ABI of the InnerProduct GEMM kernels (csrc/ip_gemm.hip): symbols, prototypes against the header, the workspace query and the
host-side refusals (no GPU: every call here returns before anything touches a device)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_ip_gemm_fwd_f32", "fcn_ip_gemm_fwd_f16", "fcn_ip_gemm_bwd_data_f32", "fcn_ip_gemm_bwd_weights_f32")
X, W, B, Y, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000      # fake, never dereferenced, 16-byte aligned
RELU, ACCUM, OUT_F32, NT = 1, 4, 8, 256
SPLIT = dict(M=40, K=18432, N=4)                                         # one output tile: the reduction is cut into slices


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for n in NAMES + ("fcn_ip_gemm_workspace_bytes",):
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
    assert re.search(r"\bsize_t\s+fcn_ip_gemm_workspace_bytes\s*\(\s*int M, int K, int N, int esize\s*\)\s*;", txt)
    assert L.PROTOTYPES["fcn_ip_gemm_workspace_bytes"] == (C.c_size_t, [C.c_int] * 4)


def test_the_argument_lists_mirror_the_streaming_kernels():
    """the engine's call sites differ only in the name (the weight gradient gains the workspace in front of the stream)"""
    for n in NAMES[:3]:
        assert L.PROTOTYPES[n] == L.PROTOTYPES[n.replace("ip_gemm", "inner_product")], n
    res, args = L.PROTOTYPES["fcn_inner_product_bwd_weights_f32"]
    assert L.PROTOTYPES["fcn_ip_gemm_bwd_weights_f32"] == (res, args[:-1] + [C.c_void_p, args[-1]])


def test_workspace_query():
    ws = L.load().fcn_ip_gemm_workspace_bytes
    for bad in ((0, 256, 4, 4), (-1, 256, 4, 4), (33, 0, 4, 4), (33, 256, 0, 4), (33, 256, -4, 4), (40, 18432, 4, 3), (40, 18432, 4, 0),
                (40, 18432, 4, 8)):
        assert ws(*bad) == 0, bad
    for esize in (4, 2):
        n = ws(40, 18432, 4, esize)
        assert n > 0 and n % 16 == 0, esize
        assert n % (40 * 4 * 4) == 0 and n // (40 * 4 * 4) > 1      # whole float32 slices of the 40 x 4 output, more than one
    assert ws(40, 18432, 4, 4) == ws(40, 18432, 4, 4)
    assert ws(1024, 4096, 4096, 4) == 0 and ws(1024, 25088, 4096, 2) == 0    # enough tiles: one launch, no workspace
    assert ws(1, 18432, 4, 4) > 0                                            # any M >= 1 is legal


def fwd(name="fcn_ip_gemm_fwd_f32", x=X, xrs=512, w=W, b=B, y=Y, ycs=64, yco=0, M=33, K=512, N=40, flags=0, ws=WS):
    return getattr(L.load(), name)(x, xrs, w, b, y, ycs, yco, M, K, N, flags, ws, None)


def bwd_data(dy=Y, dycs=64, dyco=0, w=W, dx=X, dxrs=512, M=33, K=512, N=40, flags=0, ws=WS):
    return L.load().fcn_ip_gemm_bwd_data_f32(dy, dycs, dyco, w, dx, dxrs, M, K, N, flags, ws, None)


def bwd_weights(x=X, xrs=512, dy=Y, dycs=64, dyco=0, dw=W, db=B, M=33, K=512, N=40, acc=0, ws=WS):
    return L.load().fcn_ip_gemm_bwd_weights_f32(x, xrs, dy, dycs, dyco, dw, db, M, K, N, acc, ws, None)


def says(who):
    return L.load().fcn_last_error_string().decode().startswith(who)


@pytest.mark.parametrize("name", NAMES[:2])
def test_forward_refusals(name):
    split = dict(SPLIT, xrs=18432)
    for bad in (dict(x=None), dict(w=None), dict(y=None), dict(M=0), dict(K=0), dict(N=0), dict(M=-1), dict(xrs=504), dict(yco=-8), dict(yco=32),
                dict(ycs=32), dict(flags=2), dict(flags=64), dict(flags=NT), dict(ws=None, **split)):
        assert fwd(name, **bad) == E_ARG, bad
        assert says(name[4:]), bad
    if name.endswith("f32"):
        assert fwd(name, flags=OUT_F32) == E_ARG      # float32 has no other output type
    g = 4 if name.endswith("f32") else 8
    for bad in (dict(x=X + 8), dict(w=W + 4), dict(y=Y + 8), dict(b=B + 4), dict(K=512 - g // 2, N=8), dict(xrs=512 + g // 2), dict(ycs=64 + g // 2),
                dict(ws=WS + 8, **split)):
        assert fwd(name, **bad) == E_ALIGN, bad
        assert says(name[4:]), bad
    for bad in (dict(N=1 << 16, K=1 << 15, xrs=1 << 15, ycs=1 << 16), dict(xrs=1 << 27), dict(ycs=1 << 27)):
        assert fwd(name, **bad) == E_UNSUPPORTED, bad
        assert says(name[4:]), bad


def test_backward_data_refusals():
    who = "ip_gemm_bwd_data_f32"
    split = dict(M=40, K=64, dxrs=64, N=18432, dycs=18432)              # dX is one tile, the reduction over N is cut
    for bad in (dict(dy=None), dict(w=None), dict(dx=None), dict(M=0), dict(K=0), dict(N=0), dict(dxrs=508), dict(dyco=-4), dict(dyco=28),
                dict(flags=1), dict(flags=8), dict(ws=None, **split)):
        assert bwd_data(**bad) == E_ARG and says(who), bad
    for bad in (dict(dy=Y + 4), dict(w=W + 8), dict(dx=X + 4), dict(K=510), dict(dxrs=514), dict(dycs=66), dict(ws=WS + 4, **split)):
        assert bwd_data(**bad) == E_ALIGN and says(who), bad
    for bad in (dict(N=1 << 16, K=1 << 15, dxrs=1 << 15, dycs=1 << 16), dict(dycs=1 << 27), dict(dxrs=1 << 27)):
        assert bwd_data(**bad) == E_UNSUPPORTED and says(who), bad


def test_backward_weights_refusals():
    who = "ip_gemm_bwd_weights_f32"
    split = dict(M=18432, K=64, xrs=64, N=4, dycs=4)                   # dW is one tile, the reduction over M is cut
    for bad in (dict(x=None), dict(dy=None), dict(dw=None), dict(M=0), dict(K=0), dict(N=0), dict(xrs=508), dict(dyco=-4), dict(dyco=28),
                dict(acc=2), dict(acc=-1), dict(ws=None, **split)):
        assert bwd_weights(**bad) == E_ARG and says(who), bad
    for bad in (dict(x=X + 4), dict(dy=Y + 8), dict(dw=W + 4), dict(db=B + 8), dict(K=510), dict(xrs=514), dict(dycs=66), dict(ws=WS + 4, **split)):
        assert bwd_weights(**bad) == E_ALIGN and says(who), bad
    for bad in (dict(N=1 << 16, K=1 << 15, xrs=1 << 15, dycs=1 << 16), dict(M=1 << 20, xrs=1 << 12, K=1 << 12)):
        assert bwd_weights(**bad) == E_UNSUPPORTED and says(who), bad


@pytest.mark.parametrize("m", [33, 300, 4096])
def test_rows_above_the_streaming_limit_pass_the_checks(m):
    """Without a device: a call that is refused by the LAST check (the workspace of a split shape) has passed the row count.  The
    streaming entry point refuses the same call for its rows, and says where they run."""
    split = dict(K=18432, N=4, xrs=18432, ws=None)
    for name in NAMES[:2]:
        assert fwd(name, M=m, **split) == E_ARG
        assert "needs the workspace of fcn_ip_gemm_workspace_bytes" in L.load().fcn_last_error_string().decode()
        assert fwd(name.replace("ip_gemm", "inner_product"), M=m, **split) == E_UNSUPPORTED
        msg = L.load().fcn_last_error_string().decode()
        assert msg.startswith(name[4:].replace("ip_gemm", "inner_product")) and "fcn_ip_gemm_" in msg and "%d rows" % m in msg
    assert bwd_data(M=m, K=64, dxrs=64, N=18432, dycs=18432, ws=None) == E_ARG
    assert "needs the workspace" in L.load().fcn_last_error_string().decode()
