"""C ABI of the gated-Scale kernels (csrc/gate.hip): symbols, prototypes against the header, the workspace query and the host-side
refusals (no GPU: every call here returns before anything touches a device)."""
import ctypes as C
import os
import re

from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN, E_UNSUPPORTED = 1, 2, 3
NAMES = ("fcn_scale_gate_fwd_f32", "fcn_scale_gate_fwd_f16", "fcn_scale_gate_bwd_data_f32", "fcn_scale_gate_bwd_gate_f32")
X, G, R, Y, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000      # fake, never dereferenced, 16-byte aligned


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = L.load()
    for n in NAMES + ("fcn_scale_gate_workspace_bytes",):
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
    assert re.search(r"\bsize_t\s+fcn_scale_gate_workspace_bytes\s*\(\s*int N, int ppi, int C\s*\)\s*;", txt)
    assert L.PROTOTYPES["fcn_scale_gate_workspace_bytes"] == (C.c_size_t, [C.c_int] * 3)
    # the two forwards take the same arguments: the engine's call sites differ only in the name
    assert L.PROTOTYPES[NAMES[0]] == L.PROTOTYPES[NAMES[1]]


def test_workspace_query():
    ws = L.load().fcn_scale_gate_workspace_bytes
    for bad in ((0, 49, 8), (2, 0, 8), (2, 49, 0), (-1, 49, 8), (65536, 1, 8)):
        assert ws(*bad) == 0, bad
    # N images x slabs x round4(C) floats; a slab is at least the 256 / tg pixel rows of a workgroup
    assert ws(2, 1, 6) == 2 * 1 * 8 * 4 and ws(2, 300, 6) == 2 * 3 * 8 * 4 and ws(3, 300, 68) == 3 * 19 * 68 * 4 and ws(2, 49, 20) == 2 * 2 * 20 * 4
    n = ws(8, 56 * 56, 256)
    assert n % (8 * 256 * 4) == 0 and 1 < n // (8 * 256 * 4) <= 1024


def fwd(name="fcn_scale_gate_fwd_f32", x=X, g=G, r=None, y=Y, N=2, ppi=5, C_=8, xcs=16, xco=0, grs=8, rcs=0, rco=0, ycs=16, yco=0):
    return getattr(L.load(), name)(x, g, r, y, N, ppi, C_, xcs, xco, grs, rcs, rco, ycs, yco, 0, None)


def test_forward_refusals():
    for name in NAMES[:2]:
        assert fwd(name, x=None) == E_ARG and fwd(name, g=None) == E_ARG and fwd(name, y=None) == E_ARG
        assert b"null" in L.load().fcn_last_error_string()
        assert fwd(name, N=0) == E_ARG and fwd(name, ppi=-1) == E_ARG and fwd(name, C_=0) == E_ARG
        assert fwd(name, xco=16) == E_ARG and fwd(name, ycs=4) == E_ARG and fwd(name, grs=7) == E_ARG and fwd(name, r=R, rcs=4) == E_ARG
        assert fwd(name, xcs=20 if name.endswith("f16") else 18) == E_ALIGN and fwd(name, yco=4 if name.endswith("f16") else 2, ycs=32) == E_ALIGN
        assert fwd(name, x=X + 8) == E_ALIGN and fwd(name, r=R + 4, rcs=16) == E_ALIGN and fwd(name, g=G + 2) == E_ALIGN
        assert fwd(name, N=65536) == E_UNSUPPORTED and fwd(name, N=2048, ppi=1 << 20) == E_UNSUPPORTED
    assert fwd(NAMES[1], xcs=12, xco=4, C_=4) == E_ALIGN      # (a window at 4 of 12 is a float32 window: halves come in groups of 8)


def test_backward_refusals():
    lib = L.load()
    bd = lambda dy=X, g=G, dx=Y, N=2, C_=8, dcs=16, dco=0, grs=8, xcs=16, xco=0: lib.fcn_scale_gate_bwd_data_f32(
        dy, g, dx, N, 5, C_, dcs, dco, grs, xcs, xco, 0, None)
    assert bd(dy=None) == E_ARG and bd(g=None) == E_ARG and bd(dx=None) == E_ARG and bd(C_=0) == E_ARG and bd(xco=12) == E_ARG and bd(grs=7) == E_ARG
    assert bd(dcs=18) == E_ALIGN and bd(xco=2, xcs=32) == E_ALIGN and bd(dx=Y + 4) == E_ALIGN and bd(g=G + 1) == E_ALIGN
    assert bd(N=65536) == E_UNSUPPORTED
    bg = lambda dy=X, x=R, dg=G, N=2, C_=8, dcs=16, dco=0, xcs=16, xco=0, grs=8, ws=WS: lib.fcn_scale_gate_bwd_gate_f32(
        dy, x, dg, N, 5, C_, dcs, dco, xcs, xco, grs, 0, ws, None)
    assert bg(dy=None) == E_ARG and bg(x=None) == E_ARG and bg(dg=None) == E_ARG and bg(ws=None) == E_ARG and bg(C_=-1) == E_ARG
    assert bg(dco=12) == E_ARG and bg(grs=7) == E_ARG
    assert bg(xcs=18) == E_ALIGN and bg(dco=2, dcs=32) == E_ALIGN and bg(x=R + 8) == E_ALIGN and bg(ws=WS + 4) == E_ALIGN and bg(dg=G + 1) == E_ALIGN
    assert bg(N=65536) == E_UNSUPPORTED
    assert b"scale_gate_bwd_gate" in lib.fcn_last_error_string()
