"""C ABI of the activation kernels (csrc/act.hip): symbols, prototypes against the header, the mode constants, the workspace query and
the host-side refusals (no GPU: every call here returns before anything touches a device)."""
import ctypes as C
import os
import re

import act_cases as AC
from conftest import ROOT
from fcn_object_detector_amd import lib as L

E_ARG, E_ALIGN = 1, 2
NAMES = ("fcn_act_fwd_f32", "fcn_act_fwd_f16", "fcn_act_bwd_data_f32", "fcn_act_bwd_param_f32")
X, Y, K, P, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000      # fake, never dereferenced, 16-byte aligned


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fcnhip.h")).read(), flags=re.S)


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = L.load()
    for n in NAMES + ("fcn_act_workspace_bytes",):
        assert hasattr(lib, n) and n in L.PROTOTYPES, n
    assert lib.fcn_abi_version() == 2


def test_prototypes_and_modes_match_the_header():
    txt = header()
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
    assert re.search(r"\bsize_t\s+fcn_act_workspace_bytes\s*\(\s*int pixels, int C\s*\)\s*;", txt)
    assert L.PROTOTYPES["fcn_act_workspace_bytes"] == (C.c_size_t, [C.c_int] * 2)
    m = re.search(r"enum\s*\{\s*FCN_ACT_PRELU\s*=\s*(\d+)\s*,\s*FCN_ACT_TANH\s*=\s*(\d+)\s*,\s*FCN_ACT_BIAS\s*=\s*(\d+)\s*\}", txt)
    assert m and tuple(int(v) for v in m.groups()) == (L.ACT_PRELU, L.ACT_TANH, L.ACT_BIAS)
    assert L.ACT_MODES == {"PReLU": L.ACT_PRELU, "TanH": L.ACT_TANH, "Bias": L.ACT_BIAS}
    # the argument names the issue and the engines rely on, in order
    order = lambda n: [a.split()[-1].lstrip("*") for a in re.search(r"\b%s\s*\((.*?)\)" % n, txt, flags=re.S).group(1).split(",")]
    assert order(NAMES[0]) == ["x", "y", "keep", "pixels", "C", "x_cstride", "x_coffset", "y_cstride", "y_coffset", "keep_cstride", "mode", "param",
                               "param_shared", "s"]
    assert order(NAMES[1]) == [a for a in order(NAMES[0]) if not a.startswith("keep")]
    assert order(NAMES[2])[:3] == ["dy", "ref", "dx"] and order(NAMES[2])[-5:] == ["mode", "param", "param_shared", "accumulate", "s"]
    assert order(NAMES[3])[:5] == ["dy", "x", "dparam", "pixels", "C"] and order(NAMES[3])[-4:] == ["mode", "param_shared", "d_workspace", "s"]


def test_the_file_is_built_like_the_others():
    mk = open(os.path.join(ROOT, "fcn_object_detector_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bact\.hip\b", mk, flags=re.M) and "-ffp-contract=off" in mk


def test_workspace_query():
    ws = L.load().fcn_act_workspace_bytes
    for bad in ((0, 8), (49, 0), (-1, 8), (49, -3)):
        assert ws(*bad) == 0, bad
    for case in AC.CASES:      # (slabs + 1) x round4(C) floats; a slab is at least the 256 / tg pixel rows of a workgroup
        assert ws(*case) == AC.workspace_bytes(case), case
    n = ws(8 * 128 * 256, 64)
    assert n % (64 * 4) == 0 and 1 < n // (64 * 4) - 1 <= 1024


def fwd(name="fcn_act_fwd_f32", x=X, y=Y, keep=None, p=5, c=8, xcs=16, xco=0, ycs=16, yco=0, kcs=0, mode=L.ACT_PRELU, par=P, shared=0):
    if name.endswith("f16"):
        return getattr(L.load(), name)(x, y, p, c, xcs, xco, ycs, yco, mode, par, shared, None)
    return getattr(L.load(), name)(x, y, keep, p, c, xcs, xco, ycs, yco, kcs, mode, par, shared, None)


def test_forward_refusals():
    for name in NAMES[:2]:
        f16 = name.endswith("f16")
        assert fwd(name, x=None) == E_ARG and fwd(name, y=None) == E_ARG
        assert b"null" in L.load().fcn_last_error_string()
        assert fwd(name, par=None) == E_ARG and fwd(name, par=None, mode=L.ACT_BIAS) == E_ARG
        assert b"parameter" in L.load().fcn_last_error_string()
        assert fwd(name, p=0) == E_ARG and fwd(name, c=-1) == E_ARG and fwd(name, mode=3) == E_ARG
        assert fwd(name, xco=16) == E_ARG and fwd(name, ycs=4) == E_ARG and fwd(name, yco=-8) == E_ARG
        assert fwd(name, xcs=20 if f16 else 18) == E_ALIGN and fwd(name, yco=4 if f16 else 2, ycs=32) == E_ALIGN
        assert fwd(name, x=X + 8) == E_ALIGN and fwd(name, y=Y + 4) == E_ALIGN and fwd(name, par=P + 2) == E_ALIGN
    assert fwd(NAMES[1], xcs=12, xco=4, c=4) == E_ALIGN      # (a window at 4 of 12 is a float32 window: halves come in groups of 8)
    assert fwd(keep=K, kcs=4) == E_ARG and fwd(keep=K, kcs=10) == E_ALIGN and fwd(keep=K + 4, kcs=8) == E_ALIGN


def test_backward_refusals():
    lib = L.load()
    bd = lambda dy=X, ref=Y, dx=K, c=8, dcs=16, dco=0, rcs=16, rco=0, xcs=16, xco=0, mode=L.ACT_PRELU, par=P: lib.fcn_act_bwd_data_f32(
        dy, ref, dx, 5, c, dcs, dco, rcs, rco, xcs, xco, mode, par, 0, 0, None)
    assert bd(dy=None) == E_ARG and bd(dx=None) == E_ARG and bd(ref=None) == E_ARG and bd(ref=None, mode=L.ACT_TANH) == E_ARG
    assert bd(par=None) == E_ARG and bd(c=0) == E_ARG and bd(mode=9) == E_ARG and bd(xco=12) == E_ARG and bd(rco=12) == E_ARG
    assert bd(dcs=18) == E_ALIGN and bd(xco=2, xcs=32) == E_ALIGN and bd(rcs=18) == E_ALIGN and bd(dx=K + 4) == E_ALIGN and bd(ref=Y + 8) == E_ALIGN
    bp = lambda dy=X, x=Y, dp=P, c=8, dcs=16, dco=0, xcs=16, xco=0, mode=L.ACT_PRELU, ws=WS: lib.fcn_act_bwd_param_f32(
        dy, x, dp, 5, c, dcs, dco, xcs, xco, mode, 0, ws, None)
    assert bp(mode=L.ACT_TANH) == E_ARG and b"no parameter" in lib.fcn_last_error_string()
    assert bp(dy=None) == E_ARG and bp(x=None) == E_ARG and bp(dp=None) == E_ARG and bp(ws=None) == E_ARG and bp(c=-1) == E_ARG and bp(dco=12) == E_ARG
    assert bp(xcs=18) == E_ALIGN and bp(dco=2, dcs=32) == E_ALIGN and bp(x=Y + 8) == E_ALIGN and bp(ws=WS + 4) == E_ALIGN and bp(dp=P + 1) == E_ALIGN
    assert b"act_bwd_param" in lib.fcn_last_error_string()
